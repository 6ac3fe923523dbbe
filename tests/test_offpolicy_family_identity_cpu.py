"""The host mirrors of the off-policy family return the bytes they returned before they were folded into one: every oh_*, dh_*, th_*,
sh_* entry point (tests/sacarchhost at both SACARCH values) at rows 1, 33 and 257, what the stand-alone programs print after a step
of each State, and the sizes of the four kinds of learner handle from the sizing function, against the digests in the "host" section
of tests/golden/offpolicy_family_identity_parent.json, recorded with the parent's sources (tools/gen_offpolicy_family_identity.py).
The sizes are held against the device section too: the bytes brs_ddpg_learner_scratch reported there are what the sizing function
gives."""
import json
import os

import numpy as np
import pytest

import offpolicy_family_identity as ofi

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "offpolicy_family_identity_parent.json")


@pytest.mark.parametrize("group", ofi.HOST_GROUPS)
def test_host_outputs_are_bit_identical_to_the_parent_sources(group, tmp_path):
    with open(FIXTURE) as f:
        ref = json.load(f)["host"]
    got = {k: ofi.digest(a) for k, a in ofi.run_host(group, tmp_path).items()}
    assert sorted(got) == sorted(k for k in ref if k.startswith(f"host/{group}/")), "the fixture holds other outputs than the runner makes"
    differ = [k for k in got if got[k] != ref[k]]
    for k in differ:
        print(f"{k}: {got[k]} here, {ref[k]} recorded")
    assert not differ, f"{differ} differ from the parent's sources"


def test_sizing_function_gives_the_bytes_the_parent_library_allocated(tmp_path):
    with open(FIXTURE) as f:
        ref = json.load(f)["device"]
    for name, (rows, partial_len) in ofi.host_sizing(tmp_path).items():
        want = np.array([ofi.handle_bytes(int(rows), int(partial_len), b) for b in ofi.SIZE_BATCHES], np.int64)
        assert ofi.digest(want) == ref[f"sizes/{name}"], (name, rows, partial_len, want)
