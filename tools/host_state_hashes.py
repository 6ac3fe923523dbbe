#!/usr/bin/env python3
"""sha256 of every state column the host builds of the kernel source (tests/hostsim, float and double) reach on fixed inputs:
the constructed block scenarios of tests/constructed_states.py through 5 substeps (physics call) and through 2 full env
steps, and an Env03-v2 rollout of 256 envs x 60 steps under seeded random actions with auto-reset.  Run it in two checkouts
and diff the outputs: a change of brs_core.hpp that is meant to leave every lane's arithmetic alone must leave every line
alone (profiles/r09_boxbox_identity.txt).  No GPU.

    python tools/host_state_hashes.py > hashes.txt
"""
import hashlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import constructed_states as cs  # noqa: E402
from tests.hostsim.hostsim import HostSim  # noqa: E402

THREADS = min(16, os.cpu_count() or 1)
COLUMNS = ("qpos", "qvel", "warm", "time", "aux", "xquat", "xpos")


def columns(sim):
    return dict(zip(COLUMNS, (*sim.get_state(), sim.get_aux(), *sim.get_xpose())))


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:32]


def report(case, build, cols, outputs=None):
    for k, v in cols.items():
        print(f"{case:34s} {build:6s} {k:8s} {digest(v)}")
    if outputs is not None:
        print(f"{case:34s} {build:6s} {'outputs':8s} {digest(*outputs)}")


def main():
    for double in (False, True):
        build = "double" if double else "float"
        for name in ("block_robot", "edge_edge", "pinned"):
            qpos, qvel, ctrl = cs.scenario_inputs(name)
            sim = HostSim("Env03-v2", len(qpos), noise=False, double=double, threads=THREADS)
            sim.set_state(qpos, qvel); sim.physics(ctrl, 5)
            report(f"{name}: 5 substeps", build, columns(sim))
            sim.close()
            sim = HostSim("Env03-v2", len(qpos), noise=False, double=double, threads=THREADS)
            sim.reset(); sim.set_state(qpos, qvel)
            rng, outs = np.random.default_rng(41), []
            for _ in range(2):
                outs += list(sim.step(rng.uniform(-1.5, 1.5, size=(len(qpos), 2)).astype(np.float32)))
            report(f"{name}: 2 env steps", build, columns(sim), outs)
            sim.close()
        n, steps = 256, 60
        sim = HostSim("Env03-v2", n, seed=11, auto_reset=True, double=double, threads=THREADS)
        rng, h = np.random.default_rng(12), hashlib.sha256()
        h.update(sim.reset().tobytes())
        for _ in range(steps):   # every step's outputs and every step's state go into the running hash
            for a in sim.step(rng.uniform(-1, 1, size=(n, 2)).astype(np.float32)):
                h.update(np.ascontiguousarray(a).tobytes())
            for v in columns(sim).values():
                h.update(v.tobytes())
        report(f"rollout {n} envs x {steps} steps", build, columns(sim))
        print(f"{'rollout: all steps, all columns':34s} {build:6s} {'running':8s} {h.hexdigest()[:32]}")
        sim.close()


if __name__ == "__main__":
    main()
