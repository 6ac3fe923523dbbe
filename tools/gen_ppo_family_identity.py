#!/usr/bin/env python3
"""Record tests/golden/ppo_family_identity_parent.json on the GPU: shape and sha256 of every output of tests/ppo_family_identity.py
(rollout kernels, GAE, the PPO and A2C gradient and apply kernels) with the library that is loaded -- the build a later change of
brs_policy.hip / brs_learner.hip must reproduce bit for bit (tests/test_ppo_family_identity_gpu.py).  Only the public Python
classes are used, so the file runs unchanged in a checkout of the build to be recorded, or in this tree with BRS_HIP_LIB pointing
at that build's library.  Run it on the build BEFORE such a change, never after.

    python tools/gen_ppo_family_identity.py [out.json]
"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from balance_robot_mujoco_rl_amd import _lib  # noqa: E402
import ppo_family_identity as pfi  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "ppo_family_identity_parent.json")
doc = {"build_id": _lib.build_id(), "outputs": {}}
for group in pfi.GROUPS:
    first, again = pfi.run(group), pfi.run(group)
    for k, a in first.items():
        assert a.tobytes() == again[k].tobytes(), f"{k}: two runs of the same build differ"
        doc["outputs"][k] = pfi.digest(a)
    print(f"{group}: {len(first)} outputs")
json.dump(doc, open(out, "w"), indent=1)
print(f"{out}: {os.path.getsize(out)} bytes, {len(doc['outputs'])} outputs, build {doc['build_id']}")
