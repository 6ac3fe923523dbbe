"""Launch geometry on the GPU: every step kernel brs_create can select and every workgroup size it accepts (include/brs.h:
block_threads 64, 128, 192 or 256).  The rest of the GPU suite runs at the default of 64 threads, where a workgroup is one
wave; here workgroups hold up to four waves, each with its own region of the dynamic-LDS contact list.

  A  the ledger: which step kernel every (id, timestep, block_threads, BRS_ENV01_OCC1) combination launches, and which test
     below runs it.  A new instantiation without a test fails here.
  B  Env03: one code object for every workgroup size and an env's arithmetic does not depend on its lane, so outputs and
     state are bit-identical to block_threads = 64 (step, brs_physics on constructed contact states, brs_reset).
  C  Env01 family without the 256-register cap (block_threads != 64, or BRS_ENV01_OCC1=1) against the fp64 oracle.
  D  no kernel writes past row N of a caller's output buffer.
  E  the policy / GAE kernels at MFMA tile edges (n % 64 in 1..32, n < 32) against an fp64 numpy forward."""
import ctypes as C

import numpy as np
import pytest

from tests import constructed_states as cs, parity as P, test_constructed_steps_gpu as st, test_gpu_parity as gp
from tests.test_policy_kernels import _ref_gae

pytestmark = pytest.mark.gpu

BTS = (64, 128, 192, 256)
IDS = ("Env01-v1", "Env01-v2", "Env03-v1", "Env03-v2", "Env01-v3", "Env02-v1")
RUNTIME = dict(substeps=100, timestep=5e-5)   # a non-default timestep: the kernel whose model constants are arguments
OUTPUTS = ("obs", "reward", "terminated", "truncated", "terminal_obs")

# ---- A: every step kernel instantiation brs_step can launch (brs_kernels.hip: STEP_KERNELS, step_kernel_of) -> the tests
# that run it.  Names in this module are checked to exist; "gp." names live in tests/test_gpu_parity.py, "st." names in
# tests/test_constructed_steps_gpu.py: every kernel has an owner there as well, which runs it on constructed contact states.
_SHARED_RNG = "gp.test_env_step_parity_with_shared_rng"
_FLOOR, _FLOOR_RT = "st.test_env01_step_kernels_on_floor_states", "st.test_env01_runtime_constant_step_kernels_on_floor_states"
_BLOCKS = "st.test_env03_step_kernels_on_block_states"
_MODULES = {"gp.": gp, "st.": st}
KERNELS = {
    # Env01 family at 64 threads (the default): capped at 256 registers, two waves per SIMD
    "brs_step_kernel_occ2<-1>": {"gp.test_runtime_parameter_kernel_with_non_default_timestep", _FLOOR_RT},
    "brs_step_kernel_occ2<0>": {_SHARED_RNG, _FLOOR},
    "brs_step_kernel_occ2<1>": {_SHARED_RNG, "test_c_uncapped_and_capped_env01_v2_kernels_on_the_same_inputs", _FLOOR,
                                "st.test_robots_that_stay_down_through_brs_step"},
    "brs_step_kernel_occ2<4>": {_SHARED_RNG, _FLOOR},
    "brs_step_kernel_occ2<5>": {_SHARED_RNG, _FLOOR},
    # Env03 family: the same kernel at every workgroup size
    "brs_step_kernel<true, -1>": {"test_b_env03_runtime_constant_kernel_bitwise_across_workgroup_sizes", _BLOCKS},
    "brs_step_kernel<true, 2>": {"test_b_env03_folded_kernels_bitwise_across_workgroup_sizes", _BLOCKS},
    "brs_step_kernel<true, 3>": {"test_b_env03_folded_kernels_bitwise_across_workgroup_sizes", _BLOCKS,
                                 "st.test_env03_step_kernel_on_tiled_block_states_at_256_threads",
                                 "st.test_robots_that_stay_down_through_brs_step", "st.test_lane_map_on_constructed_populations"},
    # Env01 family without the register cap: block_threads != 64, or BRS_ENV01_OCC1=1
    "brs_step_kernel<false, -1>": {"test_c_uncapped_runtime_constant_kernel_vs_oracle", _FLOOR_RT},
    "brs_step_kernel<false, 0>": {"test_c_uncapped_env01_kernels_vs_oracle", _FLOOR},
    "brs_step_kernel<false, 1>": {"test_c_uncapped_env01_kernels_vs_oracle", "test_c_occ1_switch_launches_the_128_thread_kernel",
                                  "test_c_uncapped_and_capped_env01_v2_kernels_on_the_same_inputs", _FLOOR},
    "brs_step_kernel<false, 4>": {"test_c_uncapped_env01_kernels_vs_oracle", _FLOOR},
    "brs_step_kernel<false, 5>": {"test_c_uncapped_env01_kernels_vs_oracle", _FLOOR},
}


def _exercised(kernel, test):
    """part B / C: the kernel a test just ran is in the ledger, assigned to that test"""
    assert test in KERNELS.get(kernel, ()), f"{test} ran {kernel}; the ledger assigns it to {KERNELS.get(kernel)}"


def _expected_kernel(env_id, block_threads, runtime, occ1):
    from balance_robot_mujoco_rl_amd.registry import spec
    v = -1 if runtime else spec(env_id).variant
    if env_id.startswith("Env03"):
        return f"brs_step_kernel<true, {v}>"
    if block_threads == 64 and not occ1:
        return f"brs_step_kernel_occ2<{v}>"
    return f"brs_step_kernel<false, {v}>"


def test_a_every_step_kernel_is_in_the_ledger_and_every_geometry_launches_a_known_one(monkeypatch):
    from balance_robot_mujoco_rl_amd import BatchedSim, BrsError
    monkeypatch.delenv("BRS_ENV01_OCC1", raising=False)
    monkeypatch.delenv("BRS_NO_FOLD", raising=False)
    seen = set()
    cases = [(env_id, bt, runtime, False) for env_id in IDS for runtime in (False, True) for bt in BTS]
    cases += [(env_id, 64, runtime, True) for env_id in IDS if not env_id.startswith("Env03") for runtime in (False, True)]
    for env_id, bt, runtime, occ1 in cases:
        if occ1:
            monkeypatch.setenv("BRS_ENV01_OCC1", "1")
        sim = BatchedSim(env_id, 1, block_threads=bt, **(RUNTIME if runtime else {}))  # BrsError if brs_create fails
        monkeypatch.delenv("BRS_ENV01_OCC1", raising=False)
        name = sim.step_kernel_name()
        sim.close()
        assert name == _expected_kernel(env_id, bt, runtime, occ1), (env_id, bt, runtime, occ1, name)
        seen.add(name)
    assert seen == set(KERNELS), f"launched but not in the ledger: {seen - set(KERNELS)}; in the ledger, never launched: {set(KERNELS) - seen}"
    assert len(KERNELS) == 13
    for kernel, owners in KERNELS.items():
        for t in owners:
            assert callable(getattr(_MODULES[t[:3]], t[3:], None) if t[:3] in _MODULES else globals().get(t)), f"the ledger names a missing test {t}"
        assert any(t.startswith("st.") for t in owners), f"no test runs {kernel} on constructed contact states"
    # workgroup sizes brs_create refuses
    for bt in (32, 100, 320, 512):
        with pytest.raises(BrsError, match="block_threads"):
            BatchedSim("Env03-v2", 8, block_threads=bt)


# ---- B: Env03 results do not depend on the workgroup size (bitwise)
N_B = 3 * 256 + 64 + 37   # 869: a partial last workgroup at every size, and a partial last wave


def _lockstep(sims, steps, seed):
    """step all handles with the same actions; every output of every step bit-identical to the first handle's.  -> resets"""
    import torch
    n = sims[0].n
    obs0 = sims[0].reset().clone()
    for s in sims[1:]:
        assert torch.equal(s.reset(), obs0)
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    resets = 0
    for k in range(steps):
        a = torch.rand((n, 2), generator=g, device="cuda") * 2 - 1
        ref = [x.clone() for x in sims[0].step(a)]
        for s in sims[1:]:
            for nm, x, y in zip(OUTPUTS, ref, s.step(a)):
                assert torch.equal(x, y), f"step {k}: {nm} differs at block_threads={s.block_threads} (vs {sims[0].block_threads})"
        resets += int(ref[2].sum()) + int(ref[3].sum())
    return resets


def _same_state(sims):
    """get_state, get_aux (equal_nan: the block timer is NaN while off), get_xpose bit-identical to the first handle's"""
    ref = (sims[0].get_state(), sims[0].get_aux(), sims[0].get_xpose())
    for s in sims[1:]:
        got = (s.get_state(), s.get_aux(), s.get_xpose())
        for what, x, y in zip(("qpos", "qvel", "warm", "time"), ref[0], got[0]):
            assert np.array_equal(x, y), f"{what} differs at block_threads={s.block_threads}"
        assert np.array_equal(ref[1], got[1], equal_nan=True), f"aux differs at block_threads={s.block_threads}"
        for what, x, y in zip(("xquat", "xpos"), ref[2], got[2]):
            assert np.array_equal(x, y), f"{what} differs at block_threads={s.block_threads}"


def _sims(env_id, n, **kw):
    from balance_robot_mujoco_rl_amd import BatchedSim
    sims = []
    for bt in BTS:
        s = BatchedSim(env_id, n, block_threads=bt, **kw)
        s.block_threads = bt
        sims.append(s)
    return sims


@pytest.mark.parametrize("env_id", ["Env03-v2", "Env03-v1"])
def test_b_env03_folded_kernels_bitwise_across_workgroup_sizes(env_id):
    """lane grouping on, auto-reset on (episodes of at most 40 steps), 90 steps of seeded random actions"""
    sims = _sims(env_id, N_B, seed=11, auto_reset=True, max_episode_steps=40)
    names = {s.step_kernel_name() for s in sims}
    assert len(names) == 1, names
    _exercised(names.pop(), "test_b_env03_folded_kernels_bitwise_across_workgroup_sizes")
    resets = _lockstep(sims, 90, seed=5)
    _same_state(sims)
    assert resets > 0, "the run must exercise auto-reset"
    for s in sims:
        s.close()


def test_b_env03_runtime_constant_kernel_bitwise_across_workgroup_sizes():
    sims = _sims("Env03-v2", N_B, seed=4, auto_reset=True, max_episode_steps=40, **RUNTIME)
    names = {s.step_kernel_name() for s in sims}
    assert len(names) == 1, names
    _exercised(names.pop(), "test_b_env03_runtime_constant_kernel_bitwise_across_workgroup_sizes")
    resets = _lockstep(sims, 60, seed=6)
    _same_state(sims)
    assert resets > 0
    for s in sims:
        s.close()


_tile = cs.tile


def _physics_bitwise(env_id, qpos, qvel, ctrl, nsub):
    """brs_physics at every workgroup size from the same states: bit-identical to block_threads = 64"""
    sims = _sims(env_id, len(qpos), seed=0, auto_reset=False, obs_noise=False)
    for s in sims:
        s.set_state(qpos, qvel)
        s.physics(ctrl.astype(np.float32), nsub)
    _same_state(sims)
    for s in sims:
        s.close()


def _coupled_in_every_wave(qpos, qvel):
    """the oracle's block<->robot contact count of every env -> assert that every 64-lane wave holds some"""
    n = len(qpos)
    orc = P.make("oracle", "Env03-v2", n, threads=1)
    orc.set_state(qpos, qvel)
    cnt = cs.coupled_contact_count(orc, n)
    orc.close()
    per_wave = np.add.reduceat(cnt, np.arange(0, n, 64))
    assert (per_wave > 0).all(), per_wave


@pytest.mark.parametrize("which,n", [("block_robot", 96 * 3 + 37), ("edge_edge", 64 * 5 + 37), ("pinned", 96 * 3 + 37)])
def test_b_env03_physics_on_constructed_contact_states_across_workgroup_sizes(which, n):
    """constructed block<->robot states tiled so that every wave of every workgroup holds coupled contacts: bit-identical at
    every size, and within the oracle caps of test_constructed_*_on_the_hip_path at 256 threads"""
    sc = cs.SCENARIOS[which]
    idx = _tile(len(sc["states"]()[0]), n, seed=3)
    qpos, qvel, ctrl = cs.scenario_inputs(which, idx)
    _coupled_in_every_wave(qpos, qvel)
    _physics_bitwise(sc["env"], qpos, qvel, ctrl, sc["nsub"])
    cs.check_hip_caps(which, *cs.run_scenario_on("hip", which, idx, block_threads=256))


def test_b_env03_reset_across_workgroup_sizes():
    """brs_reset with a mask that picks envs from every wave, then without a mask: obs and state bit-identical at every size;
    the masked reset leaves the other envs and their obs rows alone"""
    import torch
    sims = _sims("Env03-v2", N_B, seed=9, auto_reset=False, obs_noise=False)
    _lockstep(sims, 3, seed=2)
    rng = np.random.default_rng(4)
    mask = rng.uniform(size=N_B) < 0.25
    for w in range(0, N_B, 64):
        mask[w + (w // 64) % min(64, N_B - w)] = True
    assert all(mask[w:w + 64].any() and not mask[w:w + 64].all() for w in range(0, N_B, 64))
    q_before = sims[0].get_state()[0]
    obs_before = sims[0].obs.cpu().numpy().copy()
    m = torch.from_numpy(mask.astype(np.uint8))
    obs = [s.reset(m).cpu().numpy().copy() for s in sims]
    for s, o in zip(sims[1:], obs[1:]):
        assert np.array_equal(o, obs[0]), f"masked reset obs differ at block_threads={s.block_threads}"
    _same_state(sims)
    q_after = sims[0].get_state()[0]
    assert np.array_equal(q_after[~mask], q_before[~mask]) and np.array_equal(obs[0][~mask], obs_before[~mask])
    assert (np.abs(q_after[mask] - q_before[mask]).max(axis=1) > 1e-6).all(), "every masked env was re-drawn"
    obs = [s.reset().cpu().numpy().copy() for s in sims]
    for s, o in zip(sims[1:], obs[1:]):
        assert np.array_equal(o, obs[0]), f"reset obs differ at block_threads={s.block_threads}"
    _same_state(sims)
    for s in sims:
        s.close()


# ---- C: the Env01-family kernels without the register cap against the oracle
@pytest.mark.parametrize("env_id,bt", [("Env01-v1", 128), ("Env01-v2", 128), ("Env01-v3", 128), ("Env02-v1", 128), ("Env01-v2", 256)])
def test_c_uncapped_env01_kernels_vs_oracle(env_id, bt):
    """the assertions of test_env_step_parity_with_shared_rng at N = 2 x block_threads + 37, and G1-G3 on qpos"""
    g, kernel = gp.shared_rng_parity(env_id, 2 * bt + 37, 40, block_threads=bt)
    _exercised(kernel, "test_c_uncapped_env01_kernels_vs_oracle")
    g.check(f"{env_id} ({kernel}, {bt} threads)")
    assert g.n["up"] > 0.25 * (2 * bt + 37) * 40


def test_c_uncapped_runtime_constant_kernel_vs_oracle():
    kernel = gp.runtime_parameter_parity("Env01-v2", 2 * 128 + 37, 60, block_threads=128)
    _exercised(kernel, "test_c_uncapped_runtime_constant_kernel_vs_oracle")


def test_c_occ1_switch_launches_the_128_thread_kernel(monkeypatch):
    """BRS_ENV01_OCC1=1 at 64 threads runs <false, 1>, the kernel of 128-thread workgroups: bit-identical to it"""
    from balance_robot_mujoco_rl_amd import BatchedSim
    n = 2 * 128 + 37
    a = BatchedSim("Env01-v2", n, seed=8, auto_reset=True, max_episode_steps=25, block_threads=128)
    monkeypatch.setenv("BRS_ENV01_OCC1", "1")
    b = BatchedSim("Env01-v2", n, seed=8, auto_reset=True, max_episode_steps=25, block_threads=64)
    monkeypatch.delenv("BRS_ENV01_OCC1")
    a.block_threads, b.block_threads = 128, 64
    assert a.step_kernel_name() == b.step_kernel_name()
    _exercised(b.step_kernel_name(), "test_c_occ1_switch_launches_the_128_thread_kernel")
    assert _lockstep([a, b], 40, seed=12) > 0
    _same_state([a, b])
    a.close(); b.close()


def test_c_uncapped_and_capped_env01_v2_kernels_on_the_same_inputs():
    """<false, 1> (no register cap: spills into AGPRs) and occ2<1> (capped at 256 registers: spills to scratch) stepped in lockstep
    from the same reset.  Their floating-point instructions are the same (per-opcode counts of the gfx950 assembly differ only in
    moves, spill traffic and integer address arithmetic), so every output and the state stay bit-identical"""
    import torch
    from balance_robot_mujoco_rl_amd import BatchedSim
    n = 2 * 128 + 37
    cap = BatchedSim("Env01-v2", n, seed=10, auto_reset=True, max_episode_steps=25, block_threads=64)
    unc = BatchedSim("Env01-v2", n, seed=10, auto_reset=True, max_episode_steps=25, block_threads=128)
    cap.block_threads, unc.block_threads = 64, 128
    for s in (cap, unc):
        _exercised(s.step_kernel_name(), "test_c_uncapped_and_capped_env01_v2_kernels_on_the_same_inputs")
    assert cap.step_kernel_name() != unc.step_kernel_name()
    assert torch.equal(cap.reset(), unc.reset())
    g = torch.Generator(device="cuda"); g.manual_seed(13)
    worst, differ, resets = 0.0, [], 0
    for k in range(40):
        a = torch.rand((n, 2), generator=g, device="cuda") * 3 - 1.5
        oc = [x.clone() for x in cap.step(a)]
        ou = unc.step(a)
        differ += [f"step {k}: {nm}" for nm, x, y in zip(OUTPUTS, oc, ou) if not torch.equal(x, y)]
        worst = max(worst, float(np.abs(cap.get_state()[0] - unc.get_state()[0]).max()))
        resets += int(oc[2].sum()) + int(oc[3].sum())
    print(f"Env01-v2 uncapped <false, 1> vs occ2<1>, 40 steps in lockstep: max |dqpos| {worst:.3g}, outputs that differ: {differ[:5]}")
    assert worst == 0.0 and not differ, (worst, differ[:5])
    _same_state([cap, unc])
    assert resets > 0
    cap.close(); unc.close()


def test_c_uncapped_physics_on_floor_states_at_256_threads():
    """brs_physics<false> on the constructed floor states tiled over four waves of a 256-thread workgroup (plus a partial
    one): within the caps of test_constructed_floor_contact_states_on_the_hip_path, and bit-identical at every size"""
    sc = cs.SCENARIOS["floor"]
    idx = _tile(len(sc["states"]()[0]), 256 + 37, seed=7)
    qpos, qvel, ctrl = cs.scenario_inputs("floor", idx)
    _physics_bitwise(sc["env"], qpos, qvel, ctrl, sc["nsub"])
    cs.check_hip_caps("floor", *cs.run_scenario_on("hip", "floor", idx, block_threads=256))


# ---- D: nothing is written past row N (the C ABI as BatchedSim calls it, outputs with block_threads guard rows)
SENTINEL = 0xAB


def _buf(rows, cols, dtype):
    """[rows * cols] device buffer of `dtype` filled with SENTINEL bytes"""
    import torch
    nbytes = rows * cols * torch.empty((), dtype=dtype).element_size()
    return torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device="cuda").view(dtype)


def _guard_intact(buf, n, cols, what):
    import torch
    torch.cuda.synchronize()
    tail = buf.view(torch.uint8)[n * cols * buf.element_size():]
    assert bool((tail == SENTINEL).all()), f"{what}: written past row {n}"


def _written(buf, n, cols, what):
    import torch
    head = buf[:n * cols].view(torch.uint8).view(n, -1)
    assert bool((head != SENTINEL).any(dim=1).all()), f"{what}: a row below {n} was not written"


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("env_id,bt", [("Env01-v2", 64), ("Env01-v2", 192), ("Env03-v2", 64), ("Env03-v2", 128), ("Env03-v2", 256)])
def test_d_step_and_reset_write_nothing_past_row_n(env_id, bt):
    import torch
    from balance_robot_mujoco_rl_amd import _lib
    from balance_robot_mujoco_rl_amd.registry import spec
    L = _lib.lib()
    f32, u8 = torch.float32, torch.uint8
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for n in (1, 63, 65, bt + 1):
        cfg = _lib.BrsConfig(spec(env_id).variant, n, 0, _lib.FLAG_AUTO_RESET, 3, 0, 6, 0, 0.0, bt, 0)
        h = C.c_void_p()
        assert L.brs_create(C.byref(cfg), C.byref(h)) == 0, L.brs_last_error(None).decode()
        try:
            rows = n + bt
            obs, tobs, rew = _buf(rows, 6, f32), _buf(rows, 6, f32), _buf(rows, 1, f32)
            te, tr = _buf(rows, 1, u8), _buf(rows, 1, u8)
            act = (torch.rand((rows, 2), device="cuda") * 2 - 1).reshape(-1)
            mask = torch.ones(rows, dtype=u8, device="cuda")   # guard rows masked in: a reset that reads past N would write them
            mask[:n:2] = 0
            assert L.brs_reset(h, None, _ptr(obs), stream) == 0
            _guard_intact(obs, n, 6, f"{env_id} bt={bt} n={n} brs_reset obs")
            _written(obs, n, 6, "brs_reset obs")
            assert L.brs_reset(h, _ptr(mask), _ptr(obs), stream) == 0
            _guard_intact(obs, n, 6, f"{env_id} bt={bt} n={n} masked brs_reset obs")
            truncated = False
            for k in range(8):   # episodes of at most 6 steps: auto-reset runs inside brs_step
                assert L.brs_step(h, _ptr(act), _ptr(obs), _ptr(rew), _ptr(te), _ptr(tr), _ptr(tobs), stream) == 0, \
                    L.brs_last_error(h).decode()
                for b, cols, what in ((obs, 6, "obs"), (tobs, 6, "terminal_obs"), (rew, 1, "reward"), (te, 1, "terminated"),
                                      (tr, 1, "truncated")):
                    _guard_intact(b, n, cols, f"{env_id} bt={bt} n={n} brs_step {k} {what}")
                    _written(b, n, cols, what)
                truncated |= bool((tr[:n] == 1).any())
            assert truncated, "the time limit ended episodes"
        finally:
            L.brs_destroy(h)


def _policy_params(seed, scale=1.0):
    """flat BRS_POLICY_NPARAM float32 vector: torch.nn.Linear's default init (U(+-1/sqrt(fan_in))) times `scale` for every weight
    and bias, log_std [-0.3, 0.2]"""
    from balance_robot_mujoco_rl_amd.policy import SB3_LAYOUT
    rng = np.random.default_rng(seed)
    parts = []
    for name, shape in SB3_LAYOUT:
        if name == "log_std":
            parts.append(np.array([-0.3, 0.2]))
            continue
        fan_in = 6 if "0.weight" in name or "0.bias" in name else 64
        parts.append(rng.uniform(-1, 1, size=shape).ravel() / np.sqrt(fan_in) * scale)
    return np.concatenate(parts).astype(np.float32)


def _policy_handle(params):
    from balance_robot_mujoco_rl_amd import _lib
    L = _lib.lib()
    p = C.c_void_p()
    assert L.brs_policy_create(0, C.byref(p)) == 0
    assert L.brs_policy_set_weights(p, params.ctypes.data_as(C.POINTER(C.c_float))) == 0
    return L, p


def test_d_policy_and_gae_write_nothing_past_row_n():
    import torch
    f32, u8, G = torch.float32, torch.uint8, 256   # G: the policy / GAE kernels' workgroup size
    L, p = _policy_handle(_policy_params(1))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    try:
        for n in (1, 63, 65, G + 1):
            rows = n + G
            obs = torch.randn((rows, 6), device="cuda").reshape(-1)
            for det in (0, 1):
                a, ac, lp, v, z = _buf(rows, 2, f32), _buf(rows, 2, f32), _buf(rows, 1, f32), _buf(rows, 1, f32), _buf(rows, 2, f32)
                assert L.brs_policy_act(p, n, _ptr(obs), 7, 0, 3, det, _ptr(a), _ptr(ac), _ptr(lp), _ptr(v), _ptr(z), stream) == 0
                for b, cols, what in ((a, 2, "action"), (ac, 2, "action_clipped"), (lp, 1, "logp"), (v, 1, "value"), (z, 2, "noise")):
                    _guard_intact(b, n, cols, f"n={n} deterministic={det} brs_policy_act {what}")
                    _written(b, n, cols, what)
            v = _buf(rows, 1, f32)
            assert L.brs_policy_value(p, n, _ptr(obs), _ptr(v), stream) == 0
            _guard_intact(v, n, 1, f"n={n} brs_policy_value"); _written(v, n, 1, "value")
            # every row truncated and not terminated, guard rows too: a kernel that reads past N would bootstrap them
            term, trunc = torch.zeros(rows, dtype=u8, device="cuda"), torch.ones(rows, dtype=u8, device="cuda")
            rew = _buf(rows, 1, f32)
            rew[:n] = 0.5
            assert L.brs_rollout_bootstrap(p, n, _ptr(obs), _ptr(term), _ptr(trunc), 0.99, _ptr(rew), stream) == 0
            _guard_intact(rew, n, 1, f"n={n} brs_rollout_bootstrap")
            assert bool((rew[:n] != 0.5).all()), "every row was bootstrapped"
            T = 3
            r, val = torch.randn(T * n, device="cuda"), torch.randn(T * n, device="cuda")
            st = torch.zeros(T * n, dtype=u8, device="cuda"); st[:n] = 1
            lv, ld = torch.randn(n, device="cuda"), torch.zeros(n, dtype=u8, device="cuda")
            adv, ret = _buf(T * n + G, 1, f32), _buf(T * n + G, 1, f32)
            assert L.brs_gae(0, T, n, _ptr(r), _ptr(val), _ptr(st), _ptr(lv), _ptr(ld), 0.99, 0.95, _ptr(adv), _ptr(ret), stream) == 0
            for b, what in ((adv, "adv"), (ret, "ret")):
                _guard_intact(b, T * n, 1, f"n={n} brs_gae {what}"); _written(b, T * n, 1, what)
    finally:
        L.brs_policy_destroy(p)


# ---- E: policy kernels at tile edges against fp64
def _ref_policy(params, obs, dtype=np.float64):
    """fp64 forward of the fp32 parameters: (mean [n,2], value [n], log_std [2]); dtype=np.float32: the same numpy forward in fp32"""
    from balance_robot_mujoco_rl_amd.policy import SB3_LAYOUT
    t, off = {}, 0
    for name, shape in SB3_LAYOUT:
        k = int(np.prod(shape))
        t[name] = params[off:off + k].astype(dtype).reshape(shape)
        off += k
    x = obs.astype(dtype)

    def tower(pre, head):
        h = np.tanh(x @ t[f"mlp_extractor.{pre}.0.weight"].T + t[f"mlp_extractor.{pre}.0.bias"])
        h = np.tanh(h @ t[f"mlp_extractor.{pre}.2.weight"].T + t[f"mlp_extractor.{pre}.2.bias"])
        return h @ t[f"{head}.weight"].T + t[f"{head}.bias"]

    return tower("policy_net", "action_net"), tower("value_net", "value_net")[:, 0], t["log_std"]


TILE_EDGES = (1, 5, 31, 32, 33, 64, 96, 255, 257)
POLICY_GATE = 1e-5            # the project's policy gate: |x - ref| <= 1e-5 max(1, |ref|)
POLICY_WEIGHT_SETS = ("init", "x3", "trained")


def _policy_weight_set(kind):
    """init: torch's default init, where fast_tanh stays near its linear range; x3: the same times three (the weight set of the newer
    network kernels: the tanh saturates); trained: the dequantised weights of tests/golden/robot_move_policy.npz
    (tests/quant_policy.py: float_params("mean")) with the value tower set to zero"""
    if kind == "trained":
        from balance_robot_mujoco_rl_amd.policy import SB3_LAYOUT
        from tests.quant_policy import QuantMovePolicy
        params, off = QuantMovePolicy().float_params("mean").copy(), 0
        for name, shape in SB3_LAYOUT:
            k = int(np.prod(shape))
            if "value_net" in name:
                params[off:off + k] = 0.0
            off += k
        return params
    return _policy_params(2, {"init": 1.0, "x3": 3.0}[kind])


def _distance(x, ref):
    """max |x - ref| / max(1, |ref|): the left side of the policy gate"""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(x - ref) / np.maximum(1.0, np.abs(ref))).max()) if ref.size else 0.0


@pytest.mark.parametrize("kind", POLICY_WEIGHT_SETS)
def test_e_policy_kernels_at_tile_edges_vs_fp64(kind):
    """act (stochastic, deterministic), value and bootstrap at n with an empty second N-tile in the last wave (n % 64 in 1..32),
    a wave smaller than one tile (n < 32) and full tiles; bootstrap also with only the last row of the batch truncated.
    init: rtol 1e-5, atol 2e-6.  x3: the policy gate |x - ref| <= 1e-5 max(1, |ref|) on mean, value, actions and bootstrap (an fp32
    numpy forward is 7.4e-7 from fp64 on 4,096 such rows: the reference has more than ten times the room).  trained: nobody has
    measured fp32 on these weights, so the gate is max(1e-5, 4 x the fp32 numpy forward's own distance on the same rows) (DESIGN.md
    7.4's rule).  The kernels' largest distance is printed next to fp32 numpy's."""
    import torch
    from balance_robot_mujoco_rl_amd.policy import DevicePolicy
    params = _policy_weight_set(kind)
    pol = DevicePolicy(device=0, seed=5, env_index_base=77)
    pol.set_weights(params)
    tol = dict(rtol=1e-5, atol=2e-6)
    half_log_2pi = 0.5 * np.log(2 * np.pi)
    rng = np.random.default_rng(8)
    worst = worst32 = 0.0
    for n in TILE_EDGES:
        obs = (rng.normal(size=(n, 6)) * np.array([1.5, 4.0, 0.5, 0.5, 0.5, 0.5])).astype(np.float32)
        mean, val, ls = _ref_policy(params, obs)
        mean32, val32, _ = _ref_policy(params, obs, np.float32)
        assert mean32.dtype == val32.dtype == np.float32
        d32 = max(_distance(mean32, mean), _distance(val32, val))
        worst32 = max(worst32, d32)
        bound = POLICY_GATE if kind == "x3" else max(POLICY_GATE, 4 * d32)
        seen = []

        def close(x, ref, what):
            seen.append(_distance(x, ref))
            if kind == "init":
                np.testing.assert_allclose(x, ref, err_msg=f"{what} n={n}", **tol)
            else:
                assert seen[-1] <= bound, (kind, what, n, seen[-1], bound, d32)
        o = torch.from_numpy(obs).cuda()
        noise = torch.empty((n, 2), dtype=torch.float32, device="cuda")
        a, ac, lp, v = [x.cpu().numpy() for x in pol.act(o, step=3, noise=noise)]
        z = noise.cpu().numpy().astype(np.float64)
        assert (z != 0).all()
        a_ref = mean + np.exp(ls) * z
        close(a, a_ref, "action")
        close(ac, np.clip(a_ref, -1, 1), "action_clipped")
        close(v, val, "value")
        np.testing.assert_allclose(lp, (-0.5 * z * z - ls - half_log_2pi).sum(1), rtol=1e-5, atol=1e-5, err_msg=f"logp n={n}")
        a, ac, lp, v = [x.cpu().numpy() for x in pol.act(o, step=4, deterministic=True, noise=noise)]
        assert not noise.any(), "deterministic: z = 0"
        close(a, mean, "deterministic action (the mean)")
        close(ac, np.clip(mean, -1, 1), "deterministic action_clipped")
        np.testing.assert_allclose(lp, np.full(n, (-ls - half_log_2pi).sum()), rtol=1e-5, atol=1e-5)
        close(v, val, "deterministic value")
        close(pol.value(o).cpu().numpy(), val, "value head")
        rew = rng.normal(size=n).astype(np.float32)
        term = (rng.uniform(size=n) < 0.2).astype(np.uint8)
        last_only = np.zeros(n, np.uint8); last_only[-1] = 1
        for trunc in ((rng.uniform(size=n) < 0.5).astype(np.uint8), last_only):
            te = term if trunc is not last_only else np.zeros(n, np.uint8)
            out = pol.bootstrap(o, torch.from_numpy(te).cuda(), torch.from_numpy(trunc).cuda(), 0.99,
                                torch.from_numpy(rew.copy()).cuda()).cpu().numpy()
            boot = (trunc == 1) & (te == 0)
            close(out[boot], rew[boot] + 0.99 * val[boot], "bootstrap")
            assert np.array_equal(out[~boot], rew[~boot]), "rows without a truncated episode keep their reward"
        worst = max(worst, max(seen))
    print(f"policy kernels, {kind} weights: largest |x - ref| / max(1, |ref|) from fp64 {worst:.3g}; fp32 numpy forward on the same rows {worst32:.3g}")
    pol.close()


NOISE_ROWS = 257
NOISE_CALLS = {   # name: (seed, env_index_base, step)
    "low words": (5, 77, 3),
    "seed high word": ((0x9e3779b9 << 32) | 5, 77, 3),
    "index wraps its low word inside the batch": (5, 2 ** 32 - 100, 3),
    "index high word": (5, 2 ** 40 + 3, 3),
    "step all ones": (5, 77, 0xffffffff),
}


def test_e_policy_noise_of_every_row_vs_philox():
    """every row of one act call of 257 rows against the generator of the simulator and the oracle: counter (step, "POLI", gid_lo,
    gid_hi), key (seed_lo, seed_hi), with non-zero bits in the high words of seed and global env index and in every bit of step.
    The two uniforms are built in float32 as the kernel builds them ((float32(o >> 8) + 0.5f) 2^-24, which rounds above 2^23: in
    fp64 the reference itself would miss the tolerance where u1 rounds next to 1, about one row in 10^4); Box-Muller in fp64 from
    those; the tolerance of test_policy_kernels' row-0 check.  The five calls differ pairwise; logp is the density of the returned z."""
    import torch
    from balance_robot_mujoco_rl_amd.policy import DevicePolicy
    from oracle import oracle as O
    n, f32 = NOISE_ROWS, np.float32
    params = _policy_params(2)
    ls = params[-2:].astype(np.float64)
    obs = torch.from_numpy((np.random.default_rng(9).normal(size=(n, 6)) * np.array([1.5, 4.0, 0.5, 0.5, 0.5, 0.5])).astype(f32)).cuda()
    got = {}
    for name, (seed, base, step) in NOISE_CALLS.items():
        pol = DevicePolicy(device=0, seed=seed, env_index_base=base)
        pol.set_weights(params)
        noise = torch.empty((n, 2), dtype=torch.float32, device="cuda")
        a, ac, lp, v = pol.act(obs, step=step, noise=noise)
        z, lp = noise.cpu().numpy(), lp.cpu().numpy()
        pol.close()
        gid = base + np.arange(n, dtype=object)
        o = np.array([O.philox([step, 0x504f4c49, int(g) & 0xffffffff, int(g) >> 32], [seed & 0xffffffff, seed >> 32]) for g in gid], np.uint32)
        if base == 2 ** 32 - 100:
            assert int(gid[99]) >> 32 == 0 and int(gid[100]) & 0xffffffff == 0 and int(gid[100]) >> 32 == 1
        u = ((o[:, :2] >> 8).astype(f32) + f32(0.5)) * f32(1.0 / 16777216.0)
        assert u.dtype == f32 and (u > 0).all() and (u <= 1).all()
        u1, u2 = u[:, 0].astype(np.float64), u[:, 1].astype(np.float64)
        r = np.sqrt(-2.0 * np.log(u1))
        ref = np.stack([r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2)], axis=1)
        err = np.abs(z - ref) - 2e-5 * np.abs(ref)
        print(f"policy noise, {name}: largest |z - ref| - 2e-5 |ref| = {err.max():.3g} (bound 2e-6), largest |z| {np.abs(z).max():.3g}")
        np.testing.assert_allclose(z, ref, rtol=2e-5, atol=2e-6, err_msg=name)
        z64 = z.astype(np.float64)
        np.testing.assert_allclose(lp, (-0.5 * z64 * z64 - ls).sum(1) - np.log(2 * np.pi), rtol=1e-5, atol=1e-5, err_msg=name + " logp")
        got[name] = z
    names = list(got)
    for i, x in enumerate(names):
        for y in names[i + 1:]:
            assert (got[x] != got[y]).any(axis=1).mean() > 0.99, f"{x!r} and {y!r} drew the same noise"


@pytest.mark.parametrize("T,N", [(1, 1), (1, 257), (2, 33), (64, 3)])
def test_e_gae_at_edges_vs_fp64(T, N):
    import torch
    from balance_robot_mujoco_rl_amd.policy import gae
    rng = np.random.default_rng(T * 1000 + N)
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for last_done_all in (False, True):
        rew = rng.normal(size=(T, N)).astype(np.float32); val = rng.normal(size=(T, N)).astype(np.float32)
        start = (rng.uniform(size=(T, N)) < 0.1).astype(np.uint8)
        start[0] = 1
        lv = rng.normal(size=N).astype(np.float32)
        ld = np.ones(N, np.uint8) if last_done_all else (rng.uniform(size=N) < 0.3).astype(np.uint8)
        adv, ret = gae(c(rew), c(val), c(start), c(lv), c(ld), 0.99, 0.95)
        adv_ref, ret_ref = _ref_gae(rew, val, start, lv, ld, 0.99, 0.95, dtype=np.float64)
        np.testing.assert_allclose(adv.cpu().numpy(), adv_ref, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(ret.cpu().numpy(), ret_ref, rtol=1e-5, atol=1e-5)
        if last_done_all and T == 1:   # one step closed by a done: adv = r - V exactly
            np.testing.assert_allclose(adv.cpu().numpy(), rew - val, rtol=0, atol=1e-6)
