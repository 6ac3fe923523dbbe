"""The episode monitor (include/brs_policy.h: brs_monitor_*) without a GPU: the numpy restatement on a case
worked by hand, the host build of the kernel source against it, the same host code as a program under the sanitizers, the C
ABI's argument checks, the SB3 episode quota, and evaluate_policy against a port of SB3's counting loop."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ref_monitor as R
from balance_robot_mujoco_rl_amd import _lib, episode_count_targets, evaluate_policy
from balance_robot_mujoco_rl_amd.monitor import EpisodeStats, median_from_histogram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_DIR = os.path.join(ROOT, "tests", "monitorhost")
GXX = ["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "balance_robot_mujoco_rl_amd", "csrc")]
ERR_ARG, ERR_HIP, ERR_STATE = -1, -2, -3


# --------------------------------------------------------------------------------------- 1. the reference, by hand
HAND = [  # reward, terminated, truncated of two envs over five steps
    ([1.0, -1.0], [0, 0], [0, 0]),
    ([2.0, -1.0], [0, 0], [0, 1]),    # env 1 reaches the time limit: return -2, length 2
    ([3.0, 4.0], [1, 0], [1, 0]),     # env 0 terminated AND truncated: return 6, length 3, counts as terminated
    ([0.5, 1.0], [0, 0], [0, 0]),
    ([0.25, 1.0], [0, 0], [1, 0]),    # env 0 reaches the time limit: return 0.75, length 2
]


def _feed(mon, steps):
    for r, te, tr in steps:
        mon.update(np.array(r, np.float32), np.array(te, np.uint8), np.array(tr, np.uint8))


def test_reference_on_a_case_worked_by_hand():
    m = R.RefMonitor(2, max_len=4, log_capacity=1)
    m.reset([1, 0])
    _feed(m, HAND)
    s = m.stats()
    assert (s.episodes, s.ended, s.terminated, s.time_limit, s.steps, s.first_running, s.pending) == (1, 3, 1, 0, 5, 0, 0)
    assert (s.sum_len, s.sum_len2, s.min_len, s.max_len) == (3, 9, 3, 3)
    assert (s.sum_ret, s.sum_ret2, s.min_ret, s.max_ret, s.running_ret) == (6.0, 36.0, 6.0, 6.0, 6.0)
    assert m.histogram().tolist() == [0, 0, 0, 1, 0] and m.median_len() == 3.0
    assert [c.tolist() for c in m.episodes()] == [[0], [6.0], [3], [0]]
    m.reset()   # every episode counts
    _feed(m, HAND)
    s = m.stats()
    assert (s.episodes, s.ended, s.terminated, s.time_limit, s.steps, s.first_running, s.pending) == (3, 3, 1, 2, 5, 0, 2)
    assert (s.sum_len, s.sum_len2, s.min_len, s.max_len) == (7, 17, 2, 3)
    assert (s.sum_ret, s.sum_ret2, s.min_ret, s.max_ret, s.running_ret) == (4.75, 40.5625, -2.0, 6.0, 6.0)
    assert m.histogram().tolist() == [0, 0, 2, 1, 0] and m.median_len() == 2.0
    assert [c.size for c in m.episodes()] == [0, 0, 0, 0]
    m = R.RefMonitor(2, max_len=2, log_capacity=0)   # length 3 is beyond the histogram: bin 0
    _feed(m, HAND)
    assert m.histogram().tolist() == [1, 0, 2]


def test_median_from_histogram():
    for lens in ([3], [1, 2], [2, 2, 5], [1, 1, 4, 6], [6] * 5 + [1] * 5):
        hist = np.bincount(lens, minlength=8)
        assert median_from_histogram(hist) == float(np.median(lens)), lens
    assert median_from_histogram(np.zeros(5)) is None
    assert median_from_histogram([3, 0, 1, 0]) is None       # three of four episodes are longer than the last bin
    assert median_from_histogram([1, 0, 3, 0]) == 2.0


# --------------------------------------------------------------------------------------- 2. host build of brs_monitor.hpp
class HostMonitor:
    """tests/monitorhost/monitorhost.cpp with EpisodeMonitor's surface"""

    def __init__(self, L, n, max_len, log_capacity):
        self.L, self.n, self.max_len = L, n, max_len
        self.h = C.c_void_p(L.mh_create(n, max_len, log_capacity))
        self.rows = 0

    def reset(self, targets=None):
        t = None if targets is None else np.ascontiguousarray(targets, np.int32)
        rc = self.L.mh_reset(self.h, None if t is None else t.ctypes.data)
        self.rows = 0 if t is None or rc else int(t.sum())
        return rc

    def update(self, reward, terminated, truncated):
        self.L.mh_update(self.h, reward.ctypes.data, terminated.ctypes.data, truncated.ctypes.data)

    def stats(self):
        s = _lib.BrsEpisodeStats()
        self.L.mh_stats(self.h, C.byref(s))
        return EpisodeStats(**{k: getattr(s, k) for k, _ in s._fields_})

    def histogram(self):
        hist = np.zeros(self.max_len + 1, np.int64)
        self.L.mh_histogram(self.h, hist.ctypes.data)
        return hist

    def median_len(self):
        return median_from_histogram(self.histogram())

    def episodes(self):
        r = self.rows
        out = np.zeros(r, np.int32), np.zeros(r, np.float64), np.zeros(r, np.int32), np.zeros(r, np.uint8)
        self.L.mh_episodes(self.h, *[a.ctypes.data for a in out])
        return out

    def close(self):
        self.L.mh_destroy(self.h)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("monitorhost") / "libmonitorhost.so")
    subprocess.check_call(GXX + ["-fPIC", "-shared", "-o", so, os.path.join(HOST_DIR, "monitorhost.cpp")])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.mh_create.restype, L.mh_create.argtypes = vp, [C.c_int, C.c_int, C.c_int]
    L.mh_destroy.restype, L.mh_destroy.argtypes = None, [vp]
    L.mh_reset.restype, L.mh_reset.argtypes = C.c_int, [vp, vp]
    for name, k in (("mh_update", 4), ("mh_stats", 2), ("mh_histogram", 2), ("mh_episodes", 5)):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = None, [vp] * k
    L.mh_stats.argtypes = [vp, C.POINTER(_lib.BrsEpisodeStats)]
    return L


def test_host_build_on_the_case_worked_by_hand(host):
    ref, m = R.RefMonitor(2, 4, 1), HostMonitor(host, 2, 4, 1)
    for targets in ([1, 0], None, [0, 0]):
        ref.reset(targets); assert m.reset(targets) == 0
        _feed(ref, HAND); _feed(m, HAND)
        R.assert_monitors_equal(m, ref)
    assert m.reset([1, -1]) == ERR_ARG and m.reset([1, 1]) == ERR_ARG   # a negative target; more than the log holds
    m.close()


@pytest.mark.parametrize("case", range(5))
@pytest.mark.parametrize("n", R.STREAM_SIZES)
def test_host_build_equals_reference_on_synthetic_streams(host, n, case):
    cases = R.target_cases(n)
    if case >= len(cases):
        return   # n = 1: the quotas 1 and n coincide
    targets = cases[case]
    m = HostMonitor(host, n, R.STREAM_MAX_LEN, 0 if targets is None else int(targets.sum()))
    assert m.reset(targets) == 0
    for t, step in enumerate(R.synthetic_stream(n)):
        if t == 20:
            m.stats()   # reading in the middle of a stream changes nothing
        m.update(*step)
    ref = R.stream_reference(n, case)
    R.assert_monitors_equal(m, ref)
    s = ref.stats()
    assert s.episodes > 0 or targets is not None and targets.sum() == 0
    if n >= 63 and targets is None:   # the streams reach every branch
        assert s.terminated > 0 and s.time_limit > 0 and s.first_running >= 0 and ref.histogram()[0] > 0 and s.min_ret < 0 < s.max_ret
    m.close()


# --------------------------------------------------------------------------------------- 3. the same code under the sanitizers
def test_stand_alone_program_is_clean_under_asan_and_ubsan(tmp_path):
    """monitorhost_main.cpp has its own main: nothing sanitized is loaded into Python.  Both builds print the same digests"""
    streams = []
    for n in R.STREAM_SIZES:
        path = tmp_path / f"stream_{n}.bin"
        with open(path, "wb") as f:
            steps = R.synthetic_stream(n)
            f.write(np.array([n, len(steps)], np.int32).tobytes())
            for r, te, tr in steps:
                f.write(r.tobytes()); f.write(te.tobytes()); f.write(tr.tobytes())
        streams.append(str(path))
    out = {}
    for name, flags in (("plain", []), ("san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        exe = str(tmp_path / f"monitorhost_{name}")
        subprocess.check_call(GXX + flags + ["-o", exe, os.path.join(HOST_DIR, "monitorhost_main.cpp")])
        r = subprocess.run([exe] + streams, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (name, r.returncode, r.stderr[-2000:])
        out[name] = r.stdout
    assert out["plain"] == out["san"]
    lines = out["plain"].splitlines()
    assert len(lines) == sum(len(R.target_cases(n)) for n in R.STREAM_SIZES)
    # the program ran the cases of the test above: its episode counts are the reference's
    want = [f"n={n} quota={-1 if t is None else int(t.sum())} episodes={R.stream_reference(n, k).stats().episodes} "
            for n in R.STREAM_SIZES for k, t in enumerate(R.target_cases(n))]
    assert all(line.startswith(w) for line, w in zip(lines, want)), (lines[:3], want[:3])


# --------------------------------------------------------------------------------------- 4. C ABI without a device
MONITOR_SYMBOLS = ("brs_monitor_create", "brs_monitor_destroy", "brs_monitor_last_error", "brs_monitor_reset", "brs_monitor_update",
                   "brs_monitor_stats", "brs_monitor_histogram", "brs_monitor_episodes")


def test_symbols_are_exported_and_in_the_table():
    L = _lib.lib()
    for name in MONITOR_SYMBOLS:
        assert hasattr(L, name) and name in _lib.SIGNATURES["brs_policy.h"] and name in _lib.SYMBOLS
    assert len([s for s in _lib.SIGNATURES["brs_policy.h"] if s.startswith("brs_monitor_")]) == 8
    assert C.sizeof(_lib.BrsEpisodeStats) == 7 * 8 + 5 * 8 + 4 * 4
    assert ("brs_monitor.hip", [], False) in _lib.UNITS


def test_argument_checks_that_need_no_device():
    L = _lib.lib()
    h = C.c_void_p(1)
    for args, why in (((0, 4, 10, 0, None), b"brs_monitor_create: null argument"),
                      ((0, 0, 10, 0, C.byref(h)), b"brs_monitor_create: n must be positive"),
                      ((0, -3, 10, 0, C.byref(h)), b"brs_monitor_create: n must be positive"),
                      ((0, 4, 0, 0, C.byref(h)), b"brs_monitor_create: max_len must be positive"),
                      ((0, 4, 10, -1, C.byref(h)), b"brs_monitor_create: log_capacity must not be negative")):
        h.value = 1
        assert L.brs_monitor_create(*args) == ERR_ARG and L.brs_monitor_last_error(None) == why
        assert args[4] is None or h.value is None   # *out is cleared
    # no handle: nothing to validate against, nothing touched
    s, buf = _lib.BrsEpisodeStats(), C.c_void_p(8)
    assert L.brs_monitor_destroy(None) == ERR_STATE and L.brs_monitor_reset(None, None, None) == ERR_STATE
    assert L.brs_monitor_update(None, buf, buf, buf, None) == ERR_STATE and L.brs_monitor_stats(None, C.byref(s), None) == ERR_STATE
    assert L.brs_monitor_histogram(None, None, None) == ERR_STATE and L.brs_monitor_episodes(None, None, None, None, None, None) == ERR_STATE


def test_create_fails_loudly_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the loud-failure path is for machines without one")
    L = _lib.lib()
    h = C.c_void_p(1)
    cfg = _lib.BrsConfig(9, 4, 0, 0, 0, 0, 0, 0, 0.0, 0, 0)
    assert L.brs_create(C.byref(cfg), C.byref(C.c_void_p())) == ERR_ARG and L.brs_policy_create(0, None) == ERR_ARG
    assert L.brs_monitor_create(0, 65, 6000, 100, C.byref(h)) == ERR_HIP and h.value is None
    msg = L.brs_monitor_last_error(None)
    assert msg.startswith(b"brs_monitor_create: no HIP device (") and msg.endswith(b"); there is no CPU fallback"), msg
    # the monitor family has a slot of its own: the other families' last errors are still theirs
    assert b"variant" in L.brs_last_error(None) and b"brs_policy_create" in L.brs_policy_last_error(None)
    from balance_robot_mujoco_rl_amd import BrsError, EpisodeMonitor
    with pytest.raises(BrsError, match="no CPU fallback"):
        EpisodeMonitor(4)


# --------------------------------------------------------------------------------------- 5. the SB3 quota
@pytest.mark.parametrize("E,n", [(10, 4), (3, 8), (64, 64), (100, 64)])
def test_episode_count_targets(E, n):
    t = episode_count_targets(E, n)
    assert t.dtype == np.int32 and t.tolist() == R.sb3_targets(E, n).tolist() and t.sum() == E
    assert t.max() - t.min() <= 1 and list(t) == sorted(t)
    with pytest.raises(ValueError):
        episode_count_targets(E, 0)


# --------------------------------------------------------------------------------------- 6. evaluate_policy against SB3's loop
@pytest.fixture(scope="module")
def sb3_on_oracle():
    """SB3's loop on Env01-v2, 8 envs, time limit 25, zero action (computed once)"""
    from fake_backend import OracleSim
    sim = OracleSim("Env01-v2", 8, seed=5, max_episode_steps=25)
    zero = np.zeros((8, 2), np.float32)

    def step(obs, t):
        obs, rew, te, tr, _ = sim.step(zero)
        return obs, rew, (te | tr).astype(bool)
    out = R.sb3_evaluate_loop(step, sim.reset, 8, 20, max_steps=3 * 25)
    sim.close()
    return out


@pytest.mark.parametrize("poll_every", [1, 32])
def test_evaluate_policy_equals_sb3_on_the_oracle(sb3_on_oracle, poll_every):
    from fake_backend import OracleSim
    rets, lens, envs, steps = sb3_on_oracle
    assert len(rets) == 20 and len(set(lens)) > 1, "the sample must hold falls and the time limit"
    sim = OracleSim("Env01-v2", 8, seed=5, max_episode_steps=25)
    sim.max_episode_steps = 25   # BatchedSim's attribute; the bound on the step count
    calls = []

    def act(obs, t):
        calls.append(t)
        return np.zeros((8, 2), np.float32)
    mon = R.RefMonitor(8, max_len=25, log_capacity=20)
    got_r, got_l = evaluate_policy(act, sim, n_eval_episodes=20, return_episode_rewards=True, poll_every=poll_every, monitor=mon)
    # the same episodes, in SB3's order: returns bit for bit
    assert got_r.dtype == np.float64 and got_r.tolist() == [float(x) for x in rets] and got_l.tolist() == [int(x) for x in lens]
    env, ret, length, tl = mon.episodes()
    assert sorted(zip(env.tolist(), ret.tolist(), length.tolist())) == sorted(zip(envs, map(float, rets), map(int, lens)))
    assert tl.any() and not tl.all() and all(l == 25 for l, f in zip(length, tl) if f)
    # stops at the first poll after the last counted episode, within the bound
    assert calls == list(range(len(calls))) and steps <= len(calls) <= 3 * 25
    assert len(calls) == min(-(-steps // poll_every) * poll_every, 3 * 25)
    sim.close()
    sim = OracleSim("Env01-v2", 8, seed=5, max_episode_steps=25); sim.max_episode_steps = 25
    mean, std = evaluate_policy(act, sim, n_eval_episodes=20, poll_every=poll_every, monitor=R.RefMonitor(8, 25, 20))
    assert (mean, std) == (float(np.mean(rets)), float(np.std(rets)))
    sim.close()


def test_evaluate_policy_raises_when_episodes_never_end():
    from balance_robot_mujoco_rl_amd import BrsError

    class Endless:
        n, max_episode_steps = 3, 4

        def reset(self):
            return np.zeros((3, 6), np.float32)

        def step(self, a):
            return np.zeros((3, 6), np.float32), np.ones(3, np.float32), np.zeros(3, np.uint8), np.zeros(3, np.uint8), None
    mon = R.RefMonitor(3, 4, 5)
    with pytest.raises(BrsError, match="have not finished"):
        evaluate_policy(lambda obs, t: None, Endless(), n_eval_episodes=5, monitor=mon)
    assert mon.steps == 2 * 4   # max(target) x max_episode_steps
