#!/usr/bin/env python3
"""Record tests/golden/step_identity_parent.npz on the GPU: what brs_step returns and leaves behind over 3 steps on 256 envs
per env id (tests/step_identity.py), with the library that is loaded -- the build a later change of the step kernel must
reproduce bit for bit (tests/test_step_identity_gpu.py).  Run it on the build BEFORE such a change, never after.

    python tools/gen_step_identity.py [out.npz]
"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from balance_robot_mujoco_rl_amd import _lib  # noqa: E402
from tests import step_identity as si  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "step_identity_parent.npz")
arrays = {"build_id": np.array(_lib.build_id())}
for env_id in si.IDS:
    on, off = si.run(env_id, True), si.run(env_id, False)
    for k in si.OUTPUTS + si.STATE:
        assert si.same_bits(on[k], off[k]), f"{env_id}: {k} differs with lane grouping"
        arrays[f"{env_id}/{k}"] = on[k]
    print(f"{env_id}: terminated per step {on['terminated'].sum(axis=1)}, finite {np.isfinite(on['qpos']).all()}")
np.savez_compressed(out, **arrays)
print(f"{out}: {os.path.getsize(out)} bytes, build {_lib.build_id()}")
