"""The episode monitor's HIP kernels (csrc/brs_monitor.hip) on the device against the numpy restatement of DESIGN.md 7.3
(tests/ref_monitor.py): on synthetic streams at the sizes where a wave (63 / 64 / 65), a workgroup (257) and the reduce kernel's
stride (1025) end, on the simulator's own outputs, inside DeviceRollout.collect, and under evaluate_policy against a port of
SB3's counting loop."""
import ctypes as C

import numpy as np
import pytest

import ref_monitor as R

pytestmark = pytest.mark.gpu


def _dev(step):
    import torch
    return [torch.from_numpy(a).cuda() for a in step]


def _snapshot(mon):
    """everything a monitor returns, as bytes"""
    s = mon.stats()
    return (s, mon.histogram().tobytes(), tuple(a.tobytes() for a in mon.episodes()))


def _run_stream(n, targets, reset_at=None):
    import torch
    from balance_robot_mujoco_rl_amd import EpisodeMonitor
    mon = EpisodeMonitor(n, device=0, max_len=R.STREAM_MAX_LEN, log_capacity=0 if targets is None else int(targets.sum()))
    mon.reset(targets)
    for t, step in enumerate(R.synthetic_stream(n)):
        if t == reset_at:
            mon.reset(targets)
        if t == 20:
            mon.stats()   # reading in the middle of a stream changes nothing
        mon.update(*_dev(step))
    torch.cuda.synchronize()
    return mon


@pytest.mark.parametrize("n", R.STREAM_SIZES)
def test_kernels_equal_reference_on_synthetic_streams(n):
    for case, targets in enumerate(R.target_cases(n)):
        mon = _run_stream(n, targets)
        R.assert_monitors_equal(mon, R.stream_reference(n, case))
        first = _snapshot(mon)
        mon.close()
        again = _run_stream(n, targets)   # no floating-point atomic, a reduction of fixed shape: identical bytes
        assert _snapshot(again) == first
        again.close()


@pytest.mark.parametrize("n", [65, 1025])
def test_reset_in_the_middle_of_a_stream_zeroes_running_episodes(n):
    for case in (0, len(R.target_cases(n)) - 1):
        ref = R.stream_reference(n, case, 17)
        assert ref.stats().steps == 23 and ref.stats().ended > 0
        mon = _run_stream(n, R.target_cases(n)[case], reset_at=17)
        R.assert_monitors_equal(mon, ref)
        mon.close()


def test_one_monitor_serves_unlimited_and_target_mode_in_turn():
    n = 257
    from balance_robot_mujoco_rl_amd import EpisodeMonitor
    mon = EpisodeMonitor(n, device=0, max_len=R.STREAM_MAX_LEN, log_capacity=3 * n + 7)
    stream = [_dev(s) for s in R.synthetic_stream(n)]
    for case in (4, 0, 1, 0):
        mon.reset(R.target_cases(n)[case])
        for step in stream:
            mon.update(*step)
        R.assert_monitors_equal(mon, R.stream_reference(n, case))
    mon.close()


def test_argument_checks_with_a_handle():
    import torch
    from balance_robot_mujoco_rl_amd import BrsError, EpisodeMonitor, _lib
    L = _lib.lib()
    mon = EpisodeMonitor(4, device=0, max_len=8, log_capacity=5)
    err = lambda: L.brs_monitor_last_error(mon.h)
    i32 = lambda *v: np.array(v, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    assert L.brs_monitor_reset(mon.h, i32(1, -1, 0, 0), None) == -1 and err() == b"brs_monitor_reset: negative target"
    assert L.brs_monitor_reset(mon.h, i32(2, 2, 2, 0), None) == -1 and err() == b"brs_monitor_reset: the targets add up to more than log_capacity"
    assert L.brs_monitor_reset(mon.h, i32(2, 2, 1, 0), None) == 0
    r, f = torch.zeros(4, device="cuda"), torch.zeros(4, dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    for args in ((None, p(f), p(f)), (p(r), None, p(f)), (p(r), p(f), None)):
        assert L.brs_monitor_update(mon.h, *args, None) == -1 and err() == b"brs_monitor_update: null argument"
    assert L.brs_monitor_stats(mon.h, None, None) == -1 and err() == b"brs_monitor_stats: null argument"
    assert L.brs_monitor_histogram(mon.h, None, None) == -1 and err() == b"brs_monitor_histogram: null argument"
    assert L.brs_monitor_episodes(mon.h, None, None, None, None, None) == -1 and err() == b"brs_monitor_episodes: null argument"
    assert mon.stats().steps == 0   # none of the refused calls counted
    with pytest.raises(BrsError, match="log_capacity"):
        mon.reset([5, 1, 0, 0])
    with pytest.raises(ValueError):
        mon.reset([1, 1])
    # what crosses the ABI as a raw pointer: device, dtype, contiguity and shape
    for bad in ((r.cpu(), f, f), (r.double(), f, f), (r, f.bool(), f), (r, f, torch.zeros(8, dtype=torch.uint8, device="cuda")[::2]),
                (torch.zeros(5, device="cuda"), f, f), (r, f, f.to(torch.int32))):
        with pytest.raises(ValueError):
            mon.update(*bad)
    h = C.c_void_p()
    assert L.brs_monitor_create(1 << 20, 4, 8, 0, C.byref(h)) == -1 and b"device ordinal out of range" in L.brs_monitor_last_error(None)
    mon.close()


# --------------------------------------------------------------------------------------- on the simulator
@pytest.mark.parametrize("env_id,n,steps,max_len", [("Env01-v2", 257, 120, 25), ("Env03-v2", 65, 60, 20)])
def test_monitor_reads_the_simulators_outputs_in_place(env_id, n, steps, max_len):
    import torch
    from balance_robot_mujoco_rl_amd import BatchedSim, EpisodeMonitor, episode_count_targets
    sim = BatchedSim(env_id, n, device=0, seed=3, auto_reset=True, max_episode_steps=25)
    targets = episode_count_targets(n + 30, n)
    all_mon, some_mon = EpisodeMonitor(n, max_len=max_len), EpisodeMonitor(n, max_len=max_len, log_capacity=n + 30)
    all_ref, some_ref = R.RefMonitor(n, max_len), R.RefMonitor(n, max_len, n + 30)
    some_mon.reset(targets); some_ref.reset(targets)
    gen = torch.Generator(device="cuda").manual_seed(1)
    sim.reset()
    for _ in range(steps):
        a = torch.rand((n, 2), device="cuda", generator=gen) * 2 - 1
        _, rew, te, tr, _ = sim.step(a)
        all_mon.update(rew, te, tr); some_mon.update(rew, te, tr)
        host = rew.cpu().numpy(), te.cpu().numpy(), tr.cpu().numpy()
        all_ref.update(*host); some_ref.update(*host)
    R.assert_monitors_equal(all_mon, all_ref)
    R.assert_monitors_equal(some_mon, some_ref)
    s = all_mon.stats()
    assert s.terminated > 0 and s.time_limit > 0, s   # both ways an episode ends are in the sample
    assert s.steps == steps and some_mon.stats().pending == some_ref.stats().pending
    assert s.frac_time_limit == s.time_limit / s.episodes and abs(s.mean_ret - np.mean(all_ref.all_ret)) <= 1e-12 * abs(s.mean_ret)
    assert abs(s.std_ret - np.std(all_ref.all_ret)) <= 1e-9 * max(1.0, s.std_ret) and s.mean_len == np.mean(all_ref.all_len)
    for m in (all_mon, some_mon, sim):
        m.close()


def _policy(seed=0):
    from balance_robot_mujoco_rl_amd import _lib
    from balance_robot_mujoco_rl_amd.policy import DevicePolicy
    pol = DevicePolicy(device=0, seed=seed)
    pol.set_weights(np.random.default_rng(seed).normal(0.0, 0.3, _lib.POLICY_NPARAM).astype(np.float32))
    return pol


def test_device_rollout_with_a_monitor_changes_no_buffer():
    import torch
    from balance_robot_mujoco_rl_amd import BatchedSim, EpisodeMonitor
    from balance_robot_mujoco_rl_amd.policy import DeviceRollout
    n, T = 129, 16
    mk = lambda: BatchedSim("Env01-v2", n, device=0, seed=9, auto_reset=True, max_episode_steps=25)
    sims, pols = [mk(), mk(), mk()], [_policy(4), _policy(4)]
    mon, replay = EpisodeMonitor(n, max_len=25), EpisodeMonitor(n, max_len=25)
    plain, watched = DeviceRollout(sims[0], pols[0], T), DeviceRollout(sims[1], pols[1], T, monitor=mon)
    assert plain.monitor is None
    sims[2].reset()
    for _ in range(3):
        plain.collect(); watched.collect()
        for name in ("obs", "action", "logp", "value", "reward", "episode_start", "adv", "ret", "_last_obs", "_last_value", "_last_start"):
            assert torch.equal(getattr(plain, name), getattr(watched, name)), name
        for t in range(T):   # the same steps once more, update called by hand
            _, rew, te, tr, _ = sims[2].step(watched.action[t].clamp(-1, 1).contiguous())
            replay.update(rew, te, tr)
    a, b = _snapshot(mon), _snapshot(replay)
    assert a == b and a[0].steps == 3 * T and a[0].episodes > 0 and a[0].time_limit > 0
    # the monitor sees the env's own reward: the rollout buffer's copy has the bootstrap of the time limits added
    for m in sims + pols + [mon, replay]:
        m.close()


@pytest.mark.parametrize("which", ["float", "int8"])
@pytest.mark.parametrize("poll_every", [1, 32])
def test_evaluate_policy_equals_sb3_on_the_device(which, poll_every):
    import torch
    from balance_robot_mujoco_rl_amd import BatchedSim, EpisodeMonitor, QuantModel, QuantPolicy, evaluate_policy
    import qpolicy_cases as K
    n, E, limit = 64, 100, 25
    if which == "float":
        pol = _policy(2)
        act = lambda obs, t: pol.act(obs, t, deterministic=True)[1]
    else:
        pol = QuantPolicy(QuantModel.load(K.FIXTURE, "mean"), device=0)
        act = lambda obs, t: pol.act(obs)
    mk = lambda: BatchedSim("Env01-v2", n, device=0, seed=21, auto_reset=True, max_episode_steps=limit)
    sim = mk()

    def step(obs, t):
        obs, rew, te, tr, _ = sim.step(act(obs, t))
        return obs, rew.cpu().numpy(), (te | tr).bool().cpu().numpy()
    rets, lens, envs, steps = R.sb3_evaluate_loop(step, sim.reset, n, E, max_steps=2 * limit)
    sim.close()
    assert len(rets) == E and min(lens) < limit and max(lens) == limit

    sim = mk()
    mon = EpisodeMonitor(n, device=0, max_len=limit, log_capacity=E)
    got_r, got_l = evaluate_policy(act, sim, n_eval_episodes=E, return_episode_rewards=True, poll_every=poll_every, monitor=mon)
    assert got_r.tolist() == [float(x) for x in rets] and got_l.tolist() == [int(x) for x in lens]   # same episodes, SB3's order
    env, ret, length, _ = mon.episodes()
    assert sorted(zip(env.tolist(), ret.tolist(), length.tolist())) == sorted(zip(envs, map(float, rets), map(int, lens)))
    s = mon.stats()
    assert s.pending == 0 and s.episodes == E
    assert s.steps == min(-(-steps // poll_every) * poll_every, 2 * limit)   # the first poll after the last counted episode
    sim.close(); mon.close()
    sim = mk()
    mean, std = evaluate_policy(act, sim, n_eval_episodes=E, poll_every=poll_every)   # a monitor of its own
    assert (mean, std) == (float(np.mean(rets)), float(np.std(rets)))
    sim.close(); pol.close()
    torch.cuda.synchronize()
