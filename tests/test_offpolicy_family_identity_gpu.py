"""The kernels of the off-policy family are bit for bit what the parent build computed: the outputs of
tests/offpolicy_family_identity.py (act and q, the three targets, the critic and actor gradients without a split and at three splits
on handles of two sizes, one apply, the replay buffer, the handles' allocation sizes; both SAC architectures) against the digests in
the "device" section of tests/golden/offpolicy_family_identity_parent.json, recorded on MI355X with the build BEFORE brs_offpolicy.hip
and brs_ddpg_learner.hip took one sizing table, one call prelude, one target body and one critic-gradient launch
(tools/gen_offpolicy_family_identity.py).  A change that only moves source leaves every floating-point operation its operands and its
order, so no output may differ."""
import json
import os

import pytest

import offpolicy_family_identity as ofi

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "offpolicy_family_identity_parent.json")


@pytest.mark.gpu
@pytest.mark.parametrize("group", ofi.GROUPS)
def test_outputs_are_bit_identical_to_the_parent_build(group):
    with open(FIXTURE) as f:
        ref = json.load(f)["device"]
    got = {k: ofi.digest(a) for k, a in ofi.run(group).items()}
    assert sorted(got) == sorted(k for k in ref if k.startswith(group + "/")), "the fixture holds other outputs than the runner makes"
    differ = [k for k in got if got[k] != ref[k]]
    for k in differ:
        print(f"{k}: {got[k]} here, {ref[k]} recorded")
    assert not differ, f"{differ} differ from the parent build"
