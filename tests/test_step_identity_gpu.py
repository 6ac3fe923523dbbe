"""brs_step is bit for bit what the parent build computed: 3 steps on 256 envs (4 waves) per env id from the states of
tests/step_identity.py, obs, reward, flags, terminal_obs and the full state compared with tests/golden/step_identity_parent.npz,
recorded on MI355X with the build BEFORE the step kernel's non-arithmetic instructions were cut (tools/gen_step_identity.py;
the fixture names that build's id).  A change that only re-arranges lane masks, register moves and spills leaves every lane the
parent's floating-point operations on the parent's values, so nothing may differ, with lane grouping on and off.

The CPU test asks the oracle whether the Env03 batch holds what the comparison is about."""
import os

import numpy as np
import pytest

from tests import constructed_states as cs, parity as P, step_identity as si

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_identity_parent.npz")


@pytest.mark.gpu
@pytest.mark.parametrize("lane_grouping", [True, False], ids=["grouped", "ungrouped"])
@pytest.mark.parametrize("env_id", si.IDS)
def test_step_is_bit_identical_to_the_parent_build(env_id, lane_grouping):
    ref = np.load(FIXTURE)
    got = si.run(env_id, lane_grouping)
    differ = [k for k in si.OUTPUTS + si.STATE if not si.same_bits(got[k], ref[f"{env_id}/{k}"])]
    for k in differ:
        a, b = got[k].reshape(got[k].shape[0], -1), ref[f"{env_id}/{k}"].reshape(got[k].shape[0], -1)
        rows = np.nonzero((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1))[0]
        print(f"{env_id} {k}: {len(rows)} rows differ, first {rows[:8]}")
    assert not differ, f"{env_id}, lane grouping {lane_grouping}: {differ} differ from the parent build {ref['build_id']}"
    assert np.isfinite(got["qpos"]).all() and np.isfinite(got["qvel"]).all()


def test_env03_batch_covers_the_contact_families():
    qpos, qvel = si.env03_states()
    orc = P.make("oracle", "Env03-v2", si.N, noise=False)
    orc.reset(); orc.set_state(qpos, qvel)
    cons = [orc.forward(env=i)["contacts"] for i in range(si.N)]
    orc.close()
    floor = np.array([sum(c["body1"] == 0 and c["body2"] != 4 for c in cs_) for cs_ in cons])
    block_floor = np.array([sum(c["body1"] == 0 and c["body2"] == 4 for c in cs_) for cs_ in cons])
    wheel = np.array([sum(c["body2"] == 4 and c["body1"] in (2, 3) for c in cs_) for cs_ in cons])
    torso = np.array([sum(c["body2"] == 4 and c["body1"] == 1 for c in cs_) for cs_ in cons])
    fallen = ~P.upright(qpos)
    assert (fallen & (floor >= 4)).sum() >= 16, "fallen robots on four floor contacts (those lying on the torso's broad face)"
    assert (torso == 4).any() and (torso >= 6).any(), ("4- and 6-point torso patches", np.bincount(torso))
    from oracle import oracle as O
    edge = [O.box_box_points(cs.TS, cs.BS, q[9:12] - np.array([0, 0, 1.0]) - cs.TC, cs.quat_to_mat(q[12:16]), 0.002)[3] for q in qpos[1::4]]
    assert sum(c >= 6 for c in edge) > 16, "edge-edge points"
    assert (wheel > 0).sum() >= 16 and (block_floor >= 4).sum() >= 64, (wheel.sum(), block_floor)
    for w in range(4):   # every wave holds every family
        s = slice(64 * w, 64 * w + 64)
        assert (fallen[s] & (floor[s] >= 4)).any() and (torso[s] >= 4).any() and wheel[s].any() and block_floor[s].any()
