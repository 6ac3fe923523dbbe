"""VecNormalize (include/brs_policy.h: brs_vecnorm_*) without a GPU: the numpy restatement on a case worked by
hand, the host build of the kernel source against it on every case, the same host code as a program under the sanitizers, the
library's surface and its argument checks, and DeviceRollout's call sequence with and without a normaliser."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import ref_vecnorm as R
import vecnorm_cases as K
from balance_robot_mujoco_rl_amd import _lib

ERR_ARG, ERR_HIP, ERR_STATE = -1, -2, -3
SIZES = [n for n, _ in K.SIZES]


# --------------------------------------------------------------------------------------- 1. the reference, by hand
def _by_hand(mean, var, count, bm, bv, n):
    """update_from_moments on scalars, written out"""
    delta, tot = bm - mean, count + n
    return mean + delta * n / tot, (var * count + bv * n + delta * delta * count * n / tot) / tot, tot


def test_reference_on_a_case_worked_by_hand():
    """3 envs, 2 steps, env 1 done at the first; every observation column of env i holds the same number"""
    col = lambda *x: np.repeat(np.array(x, np.float32)[:, None], 6, axis=1)
    v = R.RefVecNormalize(3, gamma=0.5, epsilon=0.0, clip_obs=1.0, clip_reward=0.75)
    near = lambda a, b: abs(a - b) <= 4e-16 * abs(b)
    # reset: obs 1, 2, 3: mean 2, variance 2/3
    out = v.reset(col(1, 2, 3))
    m1, v1, c1 = _by_hand(0.0, 1.0, 1e-4, 2.0, 2.0 / 3.0, 3)
    assert c1 == 3.0001 and all(near(x, m1) for x in v.obs_rms.mean) and all(near(x, v1) for x in v.obs_rms.var) and v.obs_rms.count == c1
    assert abs(m1 - 2.0) < 1e-4 and abs(v1 - 2.0 / 3.0) < 2e-4   # the initial count of 1e-4 hardly weighs
    z = (np.array([1.0, 2.0, 3.0]) - m1) / math.sqrt(v1)           # about -1.22, 0, 1.22: the outer two are clipped at 1
    assert out.dtype == np.float32 and out[:, 0].tolist() == [-1.0, np.float32(z[1]), 1.0] and (out == out[:, :1]).all()
    assert v.returns.tolist() == [0, 0, 0] and v.ret_rms.count == 1e-4
    # step 1: obs 2, 4, 6 (mean 4, variance 8/3); rewards 1, 2, 3 are the returns (mean 2, variance 2/3); env 1 terminated
    te, tr = np.array([0, 1, 0], np.uint8), np.array([0, 0, 0], np.uint8)
    o, r, t = v.step(col(2, 4, 6), np.array([1, 2, 3], np.float32), te, tr, col(0, 2, 0))
    m2, v2, c2 = _by_hand(m1, v1, c1, 4.0, 8.0 / 3.0, 3)
    rm1, rv1, rc1 = _by_hand(0.0, 1.0, 1e-4, 2.0, 2.0 / 3.0, 3)
    assert near(v.obs_rms.mean[3], m2) and near(v.obs_rms.var[3], v2) and v.obs_rms.count == c2 == 6.0001
    assert near(v.ret_rms.mean, rm1) and near(v.ret_rms.var, rv1) and v.ret_rms.count == rc1
    assert abs(m2 - 3.0) < 1e-4 and abs(v2 - (2.0 / 3.0 + 8.0 / 3.0) / 2 - 1.0) < 1e-3   # pooled: mean 3, variance 5/3 + 1
    assert o[:, 0].tolist() == [np.float32((2 - m2) / math.sqrt(v2)), np.float32((4 - m2) / math.sqrt(v2)), 1.0]
    assert t[1, 0] == np.float32((2 - m2) / math.sqrt(v2)) and t[0, 0] == -1.0   # every row of terminal_obs, done or not
    assert r.tolist() == [0.75, 0.75, 0.75]                                        # 1 / sqrt(2/3) = 1.22 and more: all clipped
    assert v.returns.tolist() == [1.0, 0.0, 3.0]                                    # cleared where done, after the update
    # step 2, frozen: nothing moves but the returns' reset
    v.training = False
    before = v.stats().copy()
    o, r, t = v.step(col(3, 3, 3), np.array([0.5, -0.5, -2], np.float32), np.array([0, 0, 0], np.uint8), np.array([1, 0, 0], np.uint8), col(9, 9, 9))
    assert (v.stats() == before).all() and v.returns.tolist() == [0.0, 0.0, 3.0]
    assert r.tolist() == [np.float32(0.5 / math.sqrt(rv1)), np.float32(-0.5 / math.sqrt(rv1)), -0.75]
    # step 2 again, training: returns 1 + 0.5 * 0 ... = 0.5 gamma-discounted: [0 * .5 + 1, 0 * .5 + 1, 3 * .5 + 1]
    v.training = True
    v.step(col(3, 3, 3), np.array([1, 1, 1], np.float32), te * 0, tr, col(9, 9, 9))
    assert v.returns.tolist() == [1.0, 1.0, 2.5]                                    # mean 1.5, variance 0.5
    rm2, rv2, rc2 = _by_hand(rm1, rv1, rc1, 1.5, 0.5, 3)
    assert near(v.ret_rms.mean, rm2) and near(v.ret_rms.var, rv2) and v.ret_rms.count == rc2
    # switched off: a copy, and the return statistics still move (SB3 updates them whenever it trains)
    w = R.RefVecNormalize(3, norm_obs=False, norm_reward=False)
    x = col(5, -7, 1e6)
    assert (w.reset(x) == x).all() and w.obs_rms.count == 1e-4
    o, r, t = w.step(x, np.array([100, -100, 1], np.float32), te, tr, x)
    assert (o == x).all() and (t == x).all() and r.tolist() == [100, -100, 1] and w.obs_rms.count == 1e-4 and w.ret_rms.count == 3.0001
    # a NaN stays a NaN through the clip
    assert np.isnan(v.normalize_obs(col(np.nan))).all() and np.isnan(v.normalize_reward(np.array([np.nan], np.float32))).all()


def test_batch_moments_are_exactly_rounded():
    x = np.array([1e16, 1.0, -1e16, 1.0])   # a plain sum loses both ones
    mean, var = R.batch_moments(x)
    assert mean == 0.5 and R.batch_moments(x, "numpy")[0] != 0.5
    assert var == math.fsum((x - 0.5) ** 2) / 4


# --------------------------------------------------------------------------------------- 2. host build of brs_vecnorm.hpp
def test_cases_meet_their_conditions():
    for n in SIZES:
        c = K.case(n)
        assert c.rounds < K.ROUNDS and len(c.steps) == c.T and len(c.stats) == c.T + 1
    assert -(-65537 // 1024) == 65   # lane 0 of the fold kernel takes a second partial


def test_the_gate_of_the_statistics():
    """64 x numpy's own distance from the exactly rounded reference, floored at 1e-13 (DESIGN.md 7.13 has both numbers)"""
    y = K.yardstick()
    print(f"numpy's own mean / var against the fsum reference: {y:.3g}; gate {K.stat_gate():.3g}")
    assert 0 < y < 1e-13 / 64 * 1e3 and K.stat_gate() >= K.STAT_FLOOR


WORST = {}


@pytest.mark.parametrize("n", SIZES)
def test_host_build_against_the_reference(n):
    c, run, gate = K.case(n), K.host_run(n), K.stat_gate()
    worst = 0.0
    for k, ((outs, stats, returns), ref_outs, ref_stats, ref_returns) in enumerate(zip(run, c.out, c.stats, c.returns)):
        d = R.stat_distance(stats, ref_stats)
        worst = max(worst, d)
        assert d <= gate, (n, k, d, gate)
        assert np.array_equal(stats[12:18], ref_stats[12:18]) and stats[20] == ref_stats[20]   # the counts: exact
        assert np.array_equal(returns, ref_returns), (n, k)   # one product and one sum per env, no contraction: the same bytes
        for got, want, clip, what in zip(outs, ref_outs, (c.clip_obs, c.clip_reward, c.clip_obs), ("obs", "reward", "terminal_obs")):
            K.assert_outputs_close(got, want, clip, (n, k, what))
    WORST[n] = worst
    print(f"n = {n}: host build's largest distance from the reference {worst:.3g} (gate {gate:.3g})")


def test_host_build_frozen_switched_off_and_stateless():
    n = 257
    c = K.case(n)
    for norm_obs, norm_reward in ((True, False), (False, True), (False, False)):
        h = K.HostVecNormalize(n, norm_obs=norm_obs, norm_reward=norm_reward, clip_obs=c.clip_obs, clip_reward=c.clip_reward)
        ref = R.RefVecNormalize(n, norm_obs=norm_obs, norm_reward=norm_reward, clip_obs=c.clip_obs, clip_reward=c.clip_reward,
                                gamma=K.GAMMA, epsilon=K.EPSILON)
        K.assert_outputs_close(h.reset(c.reset_obs), ref.reset(c.reset_obs), c.clip_obs, (norm_obs, norm_reward, "reset"))
        for k, step in enumerate(c.steps):
            h.training = ref.training = k != 5   # one frozen step
            before = h.stats()
            got, want = h.step(*step), ref.step(*step)
            if k == 5:
                assert np.array_equal(h.stats(), before)
            if not norm_obs:
                assert got[0].tobytes() == step[0].tobytes() and got[2].tobytes() == step[4].tobytes()
            if not norm_reward:
                assert got[1].tobytes() == step[1].tobytes()
            for g, w, clip, what in zip(got, want, (c.clip_obs, c.clip_reward, c.clip_obs), ("obs", "reward", "terminal_obs")):
                K.assert_outputs_close(g, w, clip, (norm_obs, norm_reward, k, what))
            assert np.array_equal(h.returns(), ref.returns)
        assert R.stat_distance(h.stats(), ref.stats()) <= K.stat_gate()
        if not norm_obs:
            assert h.stats()[12] == 1e-4 and h.stats()[20] > 1e-4
        for m in (1, 65, 257):
            x = np.ascontiguousarray(c.steps[0][0][:m])
            K.assert_outputs_close(h.normalize_obs(x), ref.normalize_obs(x), c.clip_obs, (norm_obs, norm_reward, m))
        h.close()
    # stateless calls equal the step's outputs with frozen statistics, at any m
    h = K.HostVecNormalize(n, clip_obs=c.clip_obs, clip_reward=c.clip_reward)
    h.reset(c.reset_obs); h.step(*c.steps[0])
    h.training = False
    o, r, t = h.step(*c.steps[3])
    big = np.concatenate([c.steps[3][0], c.steps[3][4]])
    assert np.array_equal(h.normalize_obs(big), np.concatenate([o, t])) and np.array_equal(h.normalize_reward(c.steps[3][1]), r)
    assert np.array_equal(h.normalize_obs(big[:1]), o[:1])
    h.close()


# --------------------------------------------------------------------------------------- 3. the same code under the sanitizers
def test_stand_alone_program_is_clean_under_asan_and_ubsan(tmp_path):
    """vecnormhost_main.cpp has its own main: nothing sanitized is loaded into Python.  Both builds print the same digests"""
    streams, sizes = [], (1, 65, 257, 1025, 4097)
    for n in sizes:
        c = K.case(n)
        path = tmp_path / f"stream_{n}.bin"
        with open(path, "wb") as f:
            f.write(np.array([n, c.T], np.int32).tobytes()); f.write(np.array([c.clip_obs, c.clip_reward], np.float64).tobytes())
            f.write(c.reset_obs.tobytes())
            for step in c.steps:
                for a in step:
                    f.write(a.tobytes())
        streams.append(str(path))
    out = {}
    for name, flags in (("plain", []), ("san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        exe = str(tmp_path / f"vecnormhost_{name}")
        subprocess.check_call(K.GXX + flags + ["-o", exe, os.path.join(K.HOST_DIR, "vecnormhost_main.cpp")])
        r = subprocess.run([exe] + streams, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (name, r.returncode, r.stderr[-2000:])
        out[name] = r.stdout
    assert out["plain"] == out["san"]
    lines = out["plain"].splitlines()
    assert len(lines) == 4 * len(sizes) and len(set(lines)) == len(lines)
    # the program ran the streams of the tests above: all but the last step train
    want = [f"n={n} norm_obs={m & 1} norm_reward={m >> 1} ret_count={1e-4 + n * (K.case(n).T - 1):.4f} " for n in sizes for m in range(4)]
    assert all(line.startswith(w) for line, w in zip(lines, want)), (lines[:3], want[:3])


# --------------------------------------------------------------------------------------- 4. the library's surface
VECNORM_SYMBOLS = ("brs_vecnorm_create", "brs_vecnorm_destroy", "brs_vecnorm_last_error", "brs_vecnorm_reset", "brs_vecnorm_step",
                   "brs_vecnorm_normalize_obs", "brs_vecnorm_normalize_reward", "brs_vecnorm_get_stats", "brs_vecnorm_set_stats",
                   "brs_vecnorm_get_returns")


def test_symbols_are_exported_and_in_the_table():
    L = _lib.lib()
    for name in VECNORM_SYMBOLS:
        assert hasattr(L, name) and name in _lib.SIGNATURES["brs_policy.h"] and name in _lib.SYMBOLS
    assert sorted(s for s in _lib.SIGNATURES["brs_policy.h"] if s.startswith("brs_vecnorm_")) == sorted(VECNORM_SYMBOLS)
    assert C.sizeof(_lib.BrsVecnormStats) == 21 * 8 and C.sizeof(_lib.BrsVecnormConfig) == 4 * 8 + 2 * 4
    assert ("brs_vecnorm.hip", [], False) in _lib.UNITS


def test_argument_checks_that_need_no_device():
    L = _lib.lib()
    h = C.c_void_p(1)
    cfg = lambda co=10.0, cr=10.0: C.byref(_lib.BrsVecnormConfig(0.99, 1e-8, co, cr, 1, 1))
    for args, why in (((0, 4, cfg(), None), b"brs_vecnorm_create: null argument"),
                      ((0, 4, None, C.byref(h)), b"brs_vecnorm_create: null argument"),
                      ((0, 0, cfg(), C.byref(h)), b"brs_vecnorm_create: n must be positive"),
                      ((0, -3, cfg(), C.byref(h)), b"brs_vecnorm_create: n must be positive"),
                      ((0, 4, cfg(co=-1.0), C.byref(h)), b"brs_vecnorm_create: clip_obs must not be negative"),
                      ((0, 4, cfg(cr=-0.5), C.byref(h)), b"brs_vecnorm_create: clip_reward must not be negative"),
                      ((0, 4, cfg(cr=float("nan")), C.byref(h)), b"brs_vecnorm_create: clip_reward must not be negative")):
        h.value = 1
        assert L.brs_vecnorm_create(*args) == ERR_ARG and L.brs_vecnorm_last_error(None) == why
        assert args[3] is None or h.value is None   # *out is cleared
    # no handle: nothing to validate against, nothing touched
    s, buf = _lib.BrsVecnormStats(), C.c_void_p(8)
    assert L.brs_vecnorm_destroy(None) == ERR_STATE and L.brs_vecnorm_reset(None, buf, 1, buf, None) == ERR_STATE
    assert L.brs_vecnorm_step(None, buf, buf, buf, buf, buf, 1, buf, buf, buf, None) == ERR_STATE
    assert L.brs_vecnorm_normalize_obs(None, 1, buf, buf, None) == ERR_STATE and L.brs_vecnorm_normalize_reward(None, 0, buf, buf, None) == ERR_STATE
    assert L.brs_vecnorm_get_stats(None, C.byref(s), None) == ERR_STATE and L.brs_vecnorm_set_stats(None, C.byref(s), None) == ERR_STATE
    assert L.brs_vecnorm_get_returns(None, None, None) == ERR_STATE


def test_create_fails_loudly_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the loud-failure path is for machines without one")
    L = _lib.lib()
    h = C.c_void_p(1)
    cfg = _lib.BrsVecnormConfig(0.99, 1e-8, 10.0, 10.0, 1, 1)
    assert L.brs_policy_create(0, None) == ERR_ARG
    assert L.brs_vecnorm_create(0, 65, C.byref(cfg), C.byref(h)) == ERR_HIP and h.value is None
    msg = L.brs_vecnorm_last_error(None)
    assert msg.startswith(b"brs_vecnorm_create: no HIP device (") and msg.endswith(b"); there is no CPU fallback"), msg
    assert b"brs_policy_create" in L.brs_policy_last_error(None)   # a slot of its own
    from balance_robot_mujoco_rl_amd import BrsError, DeviceVecNormalize
    with pytest.raises(BrsError, match="the on-device VecNormalize has no CPU fallback"):
        DeviceVecNormalize(4)


def test_python_surface():
    import inspect
    import balance_robot_mujoco_rl_amd as P
    from balance_robot_mujoco_rl_amd.vecnorm import DeviceVecNormalize
    assert P.DeviceVecNormalize is DeviceVecNormalize and "DeviceVecNormalize" in P.__all__
    assert (DeviceVecNormalize._FAMILY, DeviceVecNormalize._WHAT) == ("brs_vecnorm", "the on-device VecNormalize has")
    sig = inspect.signature(DeviceVecNormalize.__init__)
    assert list(sig.parameters)[1:] == ["n", "device", "training", "norm_obs", "norm_reward", "clip_obs", "clip_reward", "gamma", "epsilon"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [True, True, True, 10.0, 10.0, 0.99, 1e-8]
    for name in ("reset", "step", "normalize_obs", "normalize_reward", "state_dict", "load_state_dict"):
        assert callable(getattr(DeviceVecNormalize, name))


# --------------------------------------------------------------------------------------- 5. DeviceRollout's call sequence
class _Log(list):
    def __call__(self, *entry):
        self.append(entry)


def _fake_rollout(normalize, monitor, T=3, n=4):
    """DeviceRollout on stand-ins that only record: the sequence of calls collect() makes, with the tensors' identities"""
    import torch
    from balance_robot_mujoco_rl_amd import policy as P
    log = _Log()
    dev = torch.device("cpu")
    names = {}

    def name(t):
        return names.get(t.data_ptr(), "rollout")

    class Sim:
        device = dev

        def __init__(self):
            self.n = n
            self.out = (torch.ones(n, 6), torch.ones(n), torch.zeros(n, dtype=torch.uint8), torch.zeros(n, dtype=torch.uint8), torch.ones(n, 6))
            for k, t in zip(("sim.obs", "sim.reward", "sim.terminated", "sim.truncated", "sim.terminal_obs"), self.out):
                names[t.data_ptr()] = k

        def reset(self):
            log("sim.reset")
            return self.out[0]

        def step(self, a):
            log("sim.step")
            return self.out

    class Pol:
        def act(self, obs, step, out):
            log("policy.act", step)

        def bootstrap(self, tobs, term, trunc, gamma, reward):
            log("policy.bootstrap", name(tobs), name(term), name(trunc))

        def value(self, obs, out):
            log("policy.value")

    class Mon:
        def update(self, rew, term, trunc):
            log("monitor.update", name(rew), name(term), name(trunc))

    class Norm:
        def __init__(self):
            self.out = (torch.full((n, 6), 2.0), torch.full((n,), 3.0), torch.full((n, 6), 4.0))
            for k, t in zip(("norm.obs", "norm.reward", "norm.terminal_obs"), self.out):
                names[t.data_ptr()] = k

        def reset(self, obs):
            log("normalize.reset", name(obs))
            return self.out[0]

        def step(self, obs, rew, term, trunc, tobs):
            log("normalize.step", *[name(x) for x in (obs, rew, term, trunc, tobs)])
            return self.out
    real_gae = P.gae
    P.gae = lambda *a: log("gae")
    try:
        kw = {} if normalize == "absent" else {"normalize": Norm() if normalize else None}
        ro = P.DeviceRollout(Sim(), Pol(), T, monitor=Mon() if monitor else None, **kw)
        ro.collect()
        first = len(log)
        ro.collect()
    finally:
        P.gae = real_gae
    return ro, list(log[:first]), list(log[first:])


@pytest.mark.parametrize("monitor", [False, True])
def test_rollout_without_a_normaliser_makes_the_calls_it_made_before(monitor):
    T = 3
    step = [("sim.step",)] + ([("monitor.update", "sim.reward", "sim.terminated", "sim.truncated")] if monitor else []) + \
           [("policy.bootstrap", "sim.terminal_obs", "sim.terminated", "sim.truncated")]
    want = [("sim.reset",)] + sum(([("policy.act", t)] + step for t in range(T)), []) + [("policy.value",), ("gae",)]
    for normalize in ("absent", None):
        ro, first, second = _fake_rollout(normalize, monitor, T)
        assert ro.normalize is None and first == want
        assert second == [(e[0], e[1] + T) if e[0] == "policy.act" else e for e in want[1:]]
        assert (ro.obs == 1).all() and (ro.reward == 1).all()


def test_rollout_with_a_normaliser_calls_in_the_order_of_the_contract():
    T = 3
    ro, first, second = _fake_rollout(True, True, T)
    step = [("sim.step",), ("monitor.update", "sim.reward", "sim.terminated", "sim.truncated"),   # the monitor: the raw reward
            ("normalize.step", "sim.obs", "sim.reward", "sim.terminated", "sim.truncated", "sim.terminal_obs"),
            ("policy.bootstrap", "norm.terminal_obs", "sim.terminated", "sim.truncated")]
    want = [("sim.reset",), ("normalize.reset", "sim.obs")] + sum(([("policy.act", t)] + step for t in range(T)), []) + [("policy.value",), ("gae",)]
    assert first == want and len(second) == len(want) - 2
    assert (ro.obs == 2).all() and (ro.reward == 3).all() and (ro._last_obs == 2).all()   # the buffer holds the normalised values


# --------------------------------------------------------------------------------------- 6. the tools' flag
def test_tools_refuse_vec_normalize_under_more_than_one_rank():
    import sys
    for tool, extra in (("train_ppo_torch.py", ["--device-rollout"]), ("train_a2c_torch.py", [])):
        r = subprocess.run([sys.executable, os.path.join(K.ROOT, "tools", tool), "--vec-normalize"] + extra, capture_output=True, text=True,
                           env=dict(os.environ, WORLD_SIZE="2"), timeout=120)
        assert r.returncode == 2 and "--vec-normalize runs on one rank only" in r.stderr, (tool, r.stderr[-500:])
    r = subprocess.run([sys.executable, os.path.join(K.ROOT, "tools", "train_ppo_torch.py"), "--vec-normalize"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--vec-normalize requires --device-rollout" in r.stderr, r.stderr[-500:]
