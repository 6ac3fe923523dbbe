#!/usr/bin/env python3
"""Second-level replay of the outliers tools/parity_locate.py dumped (GPU box): the HIP path itself, ONE substep per launch,
against the oracle from the dumped pre-step state.  parity_locate's own replay compares the kernel source on the host in
float and in double; where those two agree (the host's float rounding is not the GPU's: fast-math reciprocal / rsqrt, FMA
contraction) only the GPU can show where ITS trajectory leaves the oracle's.  For every outlier: first substep at which the
velocity difference jumps, and the oracle's contact list (body pairs) just before and after -- a jump that coincides with a
contact point appearing or disappearing is the "switches on one substep apart" mechanism of DESIGN.md 2.1.

    python tools/parity_replay_gpu.py profiles/r02_parity_config3_large.json   (rewrites the file with replay_gpu_vs_oracle added)
The replay and its first-jump rule: tests/parity.py, replay_substeps.
"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import parity as P  # noqa: E402


def main():
    path = sys.argv[1]
    rep = json.load(open(path))
    env_id = rep["env"]
    sim = P.make("hip", env_id, 1, seed=0, auto_reset=False, noise=False)
    orc = P.make("oracle", env_id, 1, seed=0, auto_reset=False, noise=False)
    for o in rep["outliers"]:
        pre = P.outlier_arrays(o["pre"])
        pairs = []
        first_jump, trace = P.replay_substeps(orc, sim, pre, pre["ctrl"], jump_abs=1e-3, jump_ratio=20, floor=1e-7,
                                              on_substep=lambda k: pairs.append(P.contact_pairs(orc, pre["ctrl"])))
        rec = dict(first_substep_dqvel_jump=first_jump, final_dqpos=trace[-1][0], final_dqvel=trace[-1][1])
        if first_jump is not None:
            lo, hi = max(0, first_jump - 2), min(250, first_jump + 2)
            rec["dqvel_before_jump"] = trace[first_jump - 1][1] if first_jump else None
            rec["dqvel_at_jump"] = trace[first_jump][1]
            rec["oracle_contact_pairs_around_jump"] = {str(k): pairs[k] for k in range(lo, hi + 1)}
            rec["oracle_contact_set_changes_within_2_substeps"] = any(pairs[k] != pairs[k + 1] for k in range(lo, hi))
        o["replay_gpu_vs_oracle"] = rec
        print(o["env"], o["step"], {k: v for k, v in rec.items() if k != "oracle_contact_pairs_around_jump"},
              rec.get("oracle_contact_pairs_around_jump"), flush=True)
    json.dump(rep, open(path, "w"), indent=1)
    sim.close(); orc.close()


if __name__ == "__main__":
    main()
