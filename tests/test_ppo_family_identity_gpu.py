"""The kernels of the MlpPolicy path are bit for bit what the parent build computed: the outputs of tests/ppo_family_identity.py
(rollout kernels at n = 257 on two weight sets, GAE, the PPO and A2C gradients at one and at two chunks per workgroup, with bad
indices and with idx null, one apply of each optimiser) against the digests in tests/golden/ppo_family_identity_parent.json,
recorded on MI355X with the build BEFORE brs_policy.hip and brs_learner.hip took their tower tiling from brs_policy_tile.hpp and
the two gradient kernels one body (tools/gen_ppo_family_identity.py; the fixture names that build's id).  A change that only moves
source leaves every floating-point operation its operands and its order, so no output may differ."""
import json
import os

import pytest

import ppo_family_identity as pfi

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppo_family_identity_parent.json")


@pytest.mark.gpu
@pytest.mark.parametrize("group", pfi.GROUPS)
def test_outputs_are_bit_identical_to_the_parent_build(group):
    with open(FIXTURE) as f:
        ref = json.load(f)
    got = {k: pfi.digest(a) for k, a in pfi.run(group).items()}
    assert sorted(got) == sorted(k for k in ref["outputs"] if k.startswith(group + "/")), "the fixture holds other outputs than the runner makes"
    differ = [k for k in got if got[k] != ref["outputs"][k]]
    for k in differ:
        print(f"{k}: {got[k]} here, {ref['outputs'][k]} recorded")
    assert not differ, f"{differ} differ from the parent build {ref['build_id']}"
