#!/usr/bin/env python3
"""Diagnostic (GPU box): one substep per launch from a dumped pre-step state, HIP path vs oracle; prints the per-dof velocity
difference and the oracle's contacts (pairs and distances) at the substeps where the difference jumps (tests/parity.py: replay_substeps).

    python tools/diag/replay_outlier_trace_gpu.py dump.json [outlier index]
"""
import json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import parity as P  # noqa: E402

rep = json.load(open(sys.argv[1]))
o = rep["outliers"][int(sys.argv[2]) if len(sys.argv) > 2 else 0]
env_id, pre = rep["env"], P.outlier_arrays(o["pre"])
sim = P.make("hip", env_id, 1, seed=0, auto_reset=False, noise=False)
orc = P.make("oracle", env_id, 1, seed=0, auto_reset=False, noise=False)
seen = dict(prev=0.0, shown=0, cons=None)
np.set_printoptions(precision=3, linewidth=200, suppress=False)


def show(k):
    """after substep k - 1: report it if the velocity difference jumped; then note the contacts entering substep k"""
    if k:
        vg, vo = sim.get_state()[1][0], orc.get_state()[1][0]
        ev = float(np.abs(vg - vo).max())
        if (ev > 1e-5 and ev > 5 * max(seen["prev"], 1e-8)) and seen["shown"] < 6:
            seen["shown"] += 1
            print(f"substep {k - 1}: max |dqvel| {ev:.3g} (before {seen['prev']:.3g}); dqvel per dof {vg - vo}")
            print(f"   oracle contacts entering the substep: {seen['cons']}; oracle qvel {vo}")
        seen["prev"] = ev
    fw = orc.forward(env=0, ctrl=(float(pre["ctrl"][0]), float(pre["ctrl"][1])))
    seen["cons"] = [(int(c["body1"]), int(c["body2"]), round(float(c["dist"]), 6)) for c in fw["contacts"]]


_, trace = P.replay_substeps(orc, sim, pre, pre["ctrl"], jump_abs=1e-5, jump_ratio=5, floor=1e-8, on_substep=show)
print("final |dqpos|", trace[-1][0])
