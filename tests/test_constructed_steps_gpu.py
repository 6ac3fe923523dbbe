"""Every step kernel brs_step can launch meets the constructed contact states (tests/constructed_states.py), teacher-forced
against the oracle over full env steps: the procedure of tests/test_constructed_steps.py on the HIP path.  The physics kernel
(brs_physics) has run these states since they exist; the step kernels are other code objects -- model constants folded at
compile time, the Env01 family capped at 256 registers at 64 threads, Env03 indexed through the lane map with the accessor
pose parked in a scratch column -- and met, until here, only what a seeded rollout from reset reaches.

  floor states         -> the Env01 family: capped (64 threads), uncapped (128), both runtime-constant kernels
  block states         -> the Env03 family: folded (Env03-v2, -v1) and runtime-constant, and 256 threads with the states tiled
  robots that stay down-> brs_step from reset with auto-reset off, 40 steps
  lane map             -> grouping on against off on populations where every env is in an expensive bucket

Each test names the kernel it ran; the ledger of tests/test_launch_geometry_gpu.py assigns every kernel to one of them."""
import numpy as np
import pytest

from tests import constructed_states as cs, parity as P

pytestmark = pytest.mark.gpu

RUNTIME = dict(substeps=100, timestep=5e-5)   # a non-default timestep: the kernels whose model constants are arguments
BLOCK = ("block_robot", "edge_edge", "pinned")
OUTPUTS = ("obs", "reward", "terminated", "truncated", "terminal_obs")


def _owned(kernel, test):
    """the kernel a test just ran is in the ledger, assigned to that test (imported here: the ledger's module imports this one)"""
    from tests import test_launch_geometry_gpu as lg
    lg._exercised(kernel, "st." + test)


@pytest.mark.parametrize("bt", [64, 128])
@pytest.mark.parametrize("env_id", ["Env01-v1", "Env01-v2", "Env01-v3", "Env02-v1"])
def test_env01_step_kernels_on_floor_states(env_id, bt):
    """robot pressed into the floor in every orientation (torso corners, wheel sides, up to the 8-slot capacity): occ2<V> at
    64 threads (256 registers, spills to scratch) and <false, V> at 128"""
    g, _, recs, kernel = cs.run_scenario_steps_on("hip", "floor", env_id, block_threads=bt)
    assert kernel.startswith("brs_step_kernel_occ2<" if bt == 64 else "brs_step_kernel<false, ") and "-1>" not in kernel, kernel
    _owned(kernel, "test_env01_step_kernels_on_floor_states")
    assert g.n["fallen"] > 0.25 * len(recs) * len(recs[0].skip), "robots that lie on the ground"


@pytest.mark.parametrize("bt", [64, 128])
def test_env01_runtime_constant_step_kernels_on_floor_states(bt):
    """100 substeps of 5e-5 s, the oracle given the same"""
    g, _, _, kernel = cs.run_scenario_steps_on("hip", "floor", block_threads=bt, **RUNTIME)
    assert kernel == ("brs_step_kernel_occ2<-1>" if bt == 64 else "brs_step_kernel<false, -1>"), kernel
    _owned(kernel, "test_env01_runtime_constant_step_kernels_on_floor_states")


@pytest.mark.parametrize("name", BLOCK)
@pytest.mark.parametrize("env_id,runtime,kernel", [("Env03-v2", False, "brs_step_kernel<true, 3>"), ("Env03-v1", False, "brs_step_kernel<true, 2>"),
                                                   ("Env03-v2", True, "brs_step_kernel<true, -1>")])
def test_env03_step_kernels_on_block_states(env_id, runtime, kernel, name):
    """6-point patches plus the wheel point, edge-edge contacts and near misses, and a block pinned between floor and robot"""
    ran = cs.run_scenario_steps_on("hip", name, env_id, **(RUNTIME if runtime else {}))[3]
    assert ran == kernel, (ran, kernel)
    _owned(ran, "test_env03_step_kernels_on_block_states")


@pytest.mark.parametrize("name", BLOCK)
def test_env03_step_kernel_on_tiled_block_states_at_256_threads(name):
    """the states tiled over four waves of a workgroup and a partial one: every wave has its own region of the contact list"""
    idx = cs.tile(len(cs.scenario_inputs(name)[0]), 256 + 37, seed=3)
    kernel = cs.run_scenario_steps_on("hip", name, index=idx, block_threads=256)[3]
    _owned(kernel, "test_env03_step_kernel_on_tiled_block_states_at_256_threads")


@pytest.mark.parametrize("env_id", ["Env03-v2", "Env01-v2"])
def test_robots_that_stay_down_through_brs_step(env_id):
    """from reset with auto-reset off: robots fall and stay down, blocks land on them, wheels
    rub on the floor -- what tests/test_gpu_parity.py::test_teacher_forced_physics_parity sends through brs_physics, with its
    action pattern (every third step zero)"""
    n, steps = 256, 40
    sim, orc = (P.make(b, env_id, n, seed=3, auto_reset=False, noise=False) for b in ("hip", "oracle"))
    kernel = sim.raw.step_kernel_name()
    _owned(kernel, "test_robots_that_stay_down_through_brs_step")
    sim.reset(); orc.reset()

    def actions(t, n, rng, obs):
        act = rng.uniform(-1, 1, size=(n, 2)).astype(np.float32)
        if t % 3 == 0:
            act[:] = 0
        return act

    g, skipped = P.Gates(), 0
    for r in P.env_steps(orc, sim, steps, actions, np.random.default_rng(5), skip=P.timer_mask):
        g.add(r.pre["qpos"], r.post_s[0], r.post_t[0], r.skip)
        skipped += int(r.skip.sum())
        assert np.isfinite(r.post_s[0]).all() and np.isfinite(r.post_s[1]).all()
    sim.close(); orc.close()
    print(f"{env_id} ({kernel}): one-sided block timers {skipped} of {n * steps} env-steps")
    g.check(f"{env_id} robots that stay down ({kernel})")
    assert skipped <= 0.02 * n * steps
    assert g.n["up"] >= 0.15 * n * steps and g.n["fallen"] >= 0.15 * n * steps, g.n


@pytest.mark.parametrize("name", BLOCK)
def test_lane_map_on_constructed_populations(name):
    """lane grouping on against off from the same set_state, 3 free-running steps with the same actions: every env of these
    populations is in an expensive cost class (there are no far lanes to fill a bucket's last wave with, and the wheel bucket
    is not diluted), and the map is still scheduling only -- everything bit-identical"""
    import torch
    from balance_robot_mujoco_rl_amd import BatchedSim
    n = 5 * 64 + 37
    qpos, qvel, _ = cs.scenario_inputs(name, cs.tile(len(cs.scenario_inputs(name)[0]), n, seed=9))
    on, off = (BatchedSim(cs.SCENARIOS[name]["env"], n, seed=2, auto_reset=False, obs_noise=False, lane_grouping=lg) for lg in (True, False))
    _owned(on.step_kernel_name(), "test_lane_map_on_constructed_populations")
    assert torch.equal(on.reset(), off.reset())
    for s in (on, off):
        s.set_state(qpos, qvel)
    gen = torch.Generator(device="cuda"); gen.manual_seed(7)
    for k in range(3):
        a = torch.rand((n, 2), generator=gen, device="cuda") * 3 - 1.5
        for nm, x, y in zip(OUTPUTS, [x.clone() for x in on.step(a)], off.step(a)):
            assert torch.equal(x, y), f"{name} step {k}: {nm} differs with lane grouping"
    for what, x, y in zip(("qpos", "qvel", "warm", "time"), on.get_state(), off.get_state()):
        assert np.array_equal(x, y), f"{name}: {what} differs with lane grouping"
        assert np.isfinite(x).all()
    assert np.array_equal(on.get_aux(), off.get_aux(), equal_nan=True), f"{name}: aux differs with lane grouping"
    for what, x, y in zip(("xquat", "xpos"), on.get_xpose(), off.get_xpose()):
        assert np.array_equal(x, y), f"{name}: {what} differs with lane grouping"
    on.close(); off.close()
