"""One wave with every case of the block<->torso generator side by side (tests/boxbox_mixed.py: edge pairs inside and outside
the margin, torso face and block face as the reference, block within reach but separated, far lanes; lane grouping off, so
the 64 envs ARE the 64 lanes in this order) on the HIP path.  The generator's arms share one tail and one pair of fp64
poses: a wave runs that code once for lanes that came through different arms.  An env's arithmetic must not depend on its
neighbours, so every lane of the mixed wave must equal, bit for bit, the same state run among 64 copies of itself -- a wave
that walks that lane's arm alone.  Plus the oracle caps of the physics call, and full env steps through the step kernels.
The host builds on the same population: tests/test_boxbox_mixed_cpu.py."""
import collections

import numpy as np
import pytest

from tests import boxbox_mixed as bm, constructed_states as cs, parity as P

pytestmark = pytest.mark.gpu


def _physics(sim, qpos, qvel, ctrl, nsub=5):
    n = len(qpos)
    sim.set_state(qpos, qvel, np.zeros((n, qvel.shape[1])), np.zeros(n))
    sim.physics(ctrl, nsub)
    return sim.get_state()


def test_every_lane_of_the_mixed_wave_equals_itself_among_copies():
    qpos, qvel, ctrl, kinds, source = bm.population()
    count = collections.Counter(kinds)
    assert sorted(count) == sorted(bm.KINDS) and min(count.values()) >= 8, count   # (which state is which kind: the CPU test)
    sim = P.make("hip", "Env03-v2", 64, noise=False, lane_grouping=False)
    orc = P.make("oracle", "Env03-v2", 64, noise=False)
    c32 = P.round_ctrl(ctrl, sim)
    mixed = [x.copy() for x in _physics(sim.raw, qpos, qvel, c32)]
    assert all(np.isfinite(x).all() for x in mixed)
    # the oracle's caps, per source scenario (the far lanes are block_robot rows)
    orc.set_state(qpos, qvel); orc.physics(c32, 5)
    vt = orc.get_state()[1]
    err = cs.rel_vel_error(vt, mixed[1])
    for name in ("block_robot", "edge_edge", "pinned"):
        cs.check_hip_caps(name, err[source == name], vt[source == name])
    # every lane against a wave of 64 copies of itself
    differ = []
    for i in range(64):
        rep = lambda a: np.repeat(a[i:i + 1], 64, axis=0)
        alone = _physics(sim.raw, rep(qpos), rep(qvel), rep(c32))
        for what, a, m in zip(("qpos", "qvel", "warm", "time"), alone, mixed):
            assert (a == a[:1]).all(), f"lane {i} ({kinds[i]}): {what} differs among 64 copies of one state"
            if not np.array_equal(a[0], m[i]):
                differ.append((i, kinds[i], what, float(np.abs(a[0] - m[i]).max())))
    sim.close(); orc.close()
    assert not differ, f"lanes whose result depends on their neighbours: {differ}"


@pytest.mark.parametrize("env_id,kernel", [("Env03-v2", "brs_step_kernel<true, 3>"), ("Env03-v1", "brs_step_kernel<true, 2>")])
def test_step_kernels_on_the_mixed_wave(env_id, kernel, monkeypatch):
    monkeypatch.setitem(cs.SCENARIOS, "boxbox_mixed", bm.scenario(env_id))
    ran = cs.run_scenario_steps_on("hip", "boxbox_mixed", env_id, lane_grouping=False)[3]
    assert ran == kernel, (ran, kernel)


def test_step_kernel_on_the_mixed_wave_at_256_threads(monkeypatch):
    """256 envs, one workgroup of four waves: each wave a different permutation of the 64 states"""
    monkeypatch.setitem(cs.SCENARIOS, "boxbox_mixed", bm.scenario())
    cs.run_scenario_steps_on("hip", "boxbox_mixed", index=cs.tile(64, 256, seed=13), block_threads=256, lane_grouping=False)
