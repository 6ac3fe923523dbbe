#!/usr/bin/env python3
"""CPU proxy of tools/parity_replay_gpu.py: replays the outliers a `parity_locate.py --student host --teacher hostdouble` run
dumped -- the kernel source on the host in FLOAT, one substep at a time, against the oracle -- and reports for each the first
substep at which the velocity difference jumps and whether the oracle's contact list (body pairs) changes within two
substeps of it.  No GPU needed: float-vs-double on the host has the same switching mechanism as GPU-vs-oracle,
minus the GPU's own rounding (fast-math reciprocal / rsqrt, FMA contraction).  The replay and its first-jump rule:
tests/parity.py, replay_substeps (called here with 1e-4 / 20x / 1e-8, this tool's own thresholds).

    python tools/parity_locate.py --student host --teacher hostdouble --env Env01-v2 --envs 2048 --steps 150 --tol 1e-5 --out /tmp/o.json
    python tools/parity_replay_host.py /tmp/o.json
"""
import collections, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import parity as P  # noqa: E402


def main():
    rep = json.load(open(sys.argv[1]))
    env_id = rep["env"]
    F = P.make("host32", env_id, 1, noise=False)
    orc = P.make("oracle", env_id, 1, seed=0, auto_reset=False, noise=False)

    cls = collections.Counter()
    for o in rep["outliers"]:
        pre = P.outlier_arrays(o["pre"])
        Pk = []
        first, _ = P.replay_substeps(orc, F, pre, pre["ctrl"], jump_abs=1e-4, jump_ratio=20, floor=1e-8,
                                     on_substep=lambda k: Pk.append(P.contact_pairs(orc, pre["ctrl"])))
        chg = None if first is None else any(Pk[k] != Pk[k + 1] for k in range(max(0, first - 2), min(250, first + 2)))
        cls["contact list changes within 2 substeps of the jump" if chg else
            ("jump with the contact list unchanged (friction rows)" if first is not None else "no jump one substep at a time")] += 1
        print(o["env"], o["step"], "tilt", round(o["tilt_deg"], 1), {k: float("%.2g" % v) for k, v in o["per_group"].items()},
              "jump at substep", first, "| contact list changes:", chg)
    print(dict(cls))


if __name__ == "__main__":
    main()
