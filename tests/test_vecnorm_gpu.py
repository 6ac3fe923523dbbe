"""VecNormalize's HIP kernels (csrc/brs_vecnorm.hip) on the device, through the C ABI: against the host build of the same source
byte for byte (statistics and returns: fp64 `+ - * /` only, contraction off on both sides) and against the numpy restatement of
DESIGN.md 7.13 (tests/ref_vecnorm.py) under the gates of tests/vecnorm_cases.py, on streams at every edge of the reduction tree;
determinism across runs, handles and streams; frozen statistics, switched-off halves, save and restore, the stateless calls,
non-finite observations, and DeviceRollout with a normaliser against the rollout recomputed from the raw quantities.

Measured on an MI355X: the fp32 outputs also equalled the host build's bytes in every case (a record, not
asserted: device fp64 sqrt and division would have to round as libm's do)."""
import ctypes as C

import numpy as np
import pytest

import ref_vecnorm as R
import vecnorm_cases as K

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 64, -12345.0
SIZES = [n for n, _ in K.SIZES]


def _ptr(t):
    return C.c_void_p(t.data_ptr())


class Guarded:
    """a float32 output of `shape` between two guard zones filled with a sentinel"""

    def __init__(self, *shape):
        import torch
        self.numel = int(np.prod(shape))
        self.buf = torch.full((self.numel + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        self.t = self.buf[GUARD:GUARD + self.numel].view(*shape)

    def numpy(self):
        host = self.buf.cpu().numpy()
        assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + self.numel:] == SENTINEL).all(), "a guard zone was written"
        return host[GUARD:GUARD + self.numel].reshape(tuple(self.t.shape)).copy()


class Abi:
    """a brs_vecnorm handle driven through the C ABI, host arrays in, host arrays out"""

    def __init__(self, n, clip_obs=10.0, clip_reward=10.0, norm_obs=True, norm_reward=True, stream=None):
        from balance_robot_mujoco_rl_amd import _lib
        self._lib, self.L, self.n, self.training = _lib, _lib.lib(), n, True
        self.stream = stream   # a torch.cuda.Stream, or None for the null stream
        cfg = _lib.BrsVecnormConfig(K.GAMMA, K.EPSILON, clip_obs, clip_reward, int(norm_obs), int(norm_reward))
        self.h = C.c_void_p()
        assert self.L.brs_vecnorm_create(0, n, C.byref(cfg), C.byref(self.h)) == 0, self.L.brs_vecnorm_last_error(None)
        self.o, self.r, self.t = Guarded(n, 6), Guarded(n), Guarded(n, 6)

    def _s(self):
        return None if self.stream is None else C.c_void_p(self.stream.cuda_stream)

    def _ok(self, rc):
        assert rc == 0, self.L.brs_vecnorm_last_error(self.h)

    def _up(self, a):
        import torch
        t = torch.tensor(a, device="cuda")   # a copy: the cases' arrays are read-only
        if self.stream is not None:
            torch.cuda.synchronize()   # the copy ran on the null stream
        return t

    def reset(self, obs):
        self._ok(self.L.brs_vecnorm_reset(self.h, _ptr(self._up(obs)), int(self.training), _ptr(self.o.t), self._s()))
        self.stats()   # waits for the stream
        return self.o.numpy()

    def step(self, obs, reward, terminated, truncated, terminal_obs):
        ins = [self._up(a) for a in (obs, reward, terminated, truncated, terminal_obs)]
        self._ok(self.L.brs_vecnorm_step(self.h, *[_ptr(t) for t in ins], int(self.training), _ptr(self.o.t), _ptr(self.r.t), _ptr(self.t.t),
                                         self._s()))
        self.stats()
        return self.o.numpy(), self.r.numpy(), self.t.numpy()

    def normalize(self, which, x):
        out, tin = Guarded(*x.shape), self._up(x)
        self._ok(getattr(self.L, "brs_vecnorm_normalize_" + which)(self.h, len(x), _ptr(tin), _ptr(out.t), self._s()))
        self.stats()
        return out.numpy()

    def stats(self):
        s = self._lib.BrsVecnormStats()
        self._ok(self.L.brs_vecnorm_get_stats(self.h, C.byref(s), self._s()))
        return np.frombuffer(bytes(s), np.float64).copy()

    def set_stats(self, a):
        s = self._lib.BrsVecnormStats.from_buffer_copy(np.ascontiguousarray(a, np.float64).tobytes())
        self._ok(self.L.brs_vecnorm_set_stats(self.h, C.byref(s), self._s()))

    def returns(self):
        r = np.zeros(self.n, np.float64)
        self._ok(self.L.brs_vecnorm_get_returns(self.h, r.ctypes.data_as(C.POINTER(C.c_double)), self._s()))
        return r

    def close(self):
        assert self.L.brs_vecnorm_destroy(self.h) == 0


def _of_case(c, **kw):
    return Abi(c.n, clip_obs=c.clip_obs, clip_reward=c.clip_reward, **kw)


def _run(v, c, first=0, reset=True):
    """the stream of a case from step `first` -> per call (outputs, stats, returns)"""
    run = [((v.reset(c.reset_obs),), v.stats(), v.returns())] if reset else []
    for step in c.steps[first:]:
        run.append((v.step(*step), v.stats(), v.returns()))
    return run


def _bytes(run):
    return [(tuple(o.tobytes() for o in outs), stats.tobytes(), returns.tobytes()) for outs, stats, returns in run]


INITIAL = np.r_[np.zeros(6), np.ones(6), np.full(6, 1e-4), 0.0, 1.0, 1e-4]


# --------------------------------------------------------------------------------------- every case through the C ABI
@pytest.mark.parametrize("n", SIZES)
def test_every_case_against_the_host_build_and_the_reference(n):
    c, host, gate = K.case(n), K.host_run(n), K.stat_gate()
    v = _of_case(c)
    assert np.array_equal(v.stats(), INITIAL) and not v.returns().any()
    run = _run(v, c)
    v.close()
    worst, same_outputs = 0.0, True
    for k, ((outs, stats, returns), (h_outs, h_stats, h_returns)) in enumerate(zip(run, host)):
        assert stats.tobytes() == h_stats.tobytes(), (n, k, "statistics differ from the host build", stats - h_stats)
        assert returns.tobytes() == h_returns.tobytes(), (n, k, "returns differ from the host build")
        d = R.stat_distance(stats, c.stats[k])
        worst = max(worst, d)
        assert d <= gate, (n, k, d, gate)
        assert np.array_equal(returns, c.returns[k])
        for got, want, h_out, clip, what in zip(outs, c.out[k], h_outs, (c.clip_obs, c.clip_reward, c.clip_obs), ("obs", "reward", "terminal_obs")):
            K.assert_outputs_close(got, want, clip, (n, k, what))
            same_outputs &= got.tobytes() == h_out.tobytes()
    print(f"n = {n}: statistics and returns equal the host build's bytes; largest distance from the reference {worst:.3g} (gate {gate:.3g}); "
          f"fp32 outputs equal the host build's bytes: {same_outputs}")


# --------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("n", [257, 4097])
def test_same_bytes_on_every_run_handle_and_stream(n):
    import torch
    c = K.case(n)
    v = _of_case(c)
    first = _bytes(_run(v, c))
    v.set_stats(INITIAL)
    assert first == _bytes(_run(v, c)), "the same stream twice on one handle"
    v.close()
    fresh = _of_case(c)
    assert first == _bytes(_run(fresh, c)), "a fresh handle"
    fresh.close()
    side = _of_case(c, stream=torch.cuda.Stream())
    assert first == _bytes(_run(side, c)), "on a second stream"
    side.close()
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------- frozen statistics
def test_frozen_statistics():
    n = 1025
    c = K.case(n)
    v = _of_case(c)
    _run(v, c)
    v.step(*c.steps[2])   # no env is done at step 2: every return is running
    stats, returns = v.stats(), v.returns()
    assert returns.all()
    v.training = False
    obs, reward, te, tr, tobs = c.steps[0]
    o, r, t = v.step(obs, reward, te, tr, tobs)
    assert v.stats().tobytes() == stats.tobytes()
    done = (te | tr) != 0
    assert done.any() and not done.all()
    assert np.array_equal(v.returns(), np.where(done, 0.0, returns))   # not advanced, cleared where done
    assert o.tobytes() == v.normalize("obs", obs).tobytes() and t.tobytes() == v.normalize("obs", tobs).tobytes()
    assert r.tobytes() == v.normalize("reward", reward).tobytes()
    assert v.reset(obs).tobytes() == o.tobytes() and v.stats().tobytes() == stats.tobytes() and not v.returns().any()
    v.close()


# --------------------------------------------------------------------------------------- switched-off halves
@pytest.mark.parametrize("norm_obs,norm_reward", [(False, True), (True, False)])
def test_a_switched_off_half_copies_through_and_leaves_the_other_alone(norm_obs, norm_reward):
    n = 257
    c = K.case(n)
    v, both = _of_case(c, norm_obs=norm_obs, norm_reward=norm_reward), _of_case(c)
    run, full = _run(v, c), _run(both, c)
    v.close(); both.close()
    assert (run[0][0][0].tobytes() == c.reset_obs.tobytes()) == (not norm_obs)
    for k, (((o, r, t), stats, returns), step) in enumerate(zip(run[1:], c.steps), 1):
        (ho, hr, ht), h_stats, h_returns = full[k]
        if norm_obs:
            assert o.tobytes() == ho.tobytes() and t.tobytes() == ht.tobytes() and r.tobytes() == step[1].tobytes()
            assert stats.tobytes() == h_stats.tobytes()
        else:
            assert o.tobytes() == step[0].tobytes() and t.tobytes() == step[4].tobytes() and r.tobytes() == hr.tobytes()
            assert np.array_equal(stats[:18], INITIAL[:18]) and stats[18:].tobytes() == h_stats[18:].tobytes()
        assert returns.tobytes() == h_returns.tobytes()   # SB3 keeps the return statistics whenever it trains


# --------------------------------------------------------------------------------------- save and restore
def test_get_stats_set_stats_and_continue():
    n = 1025
    c, whole = K.case(n), _bytes(K.host_run(1025))
    v = _of_case(c)
    run = [((v.reset(c.reset_obs),), v.stats(), v.returns())]
    for k, step in enumerate(c.steps):
        if k in (1, 4):
            v.set_stats(v.stats())
        run.append((v.step(*step), v.stats(), v.returns()))
    assert [x[1:] for x in _bytes(run)] == [x[1:] for x in whole]
    # into another handle, after the step at which every env was done (the returns are all zero, as in a new handle)
    saved = run[2][1]
    assert not run[2][2].any()
    other = _of_case(c)
    other.set_stats(saved)
    assert other.stats().tobytes() == saved.tobytes()
    rest = _run(other, c, first=2, reset=False)
    assert [x[1:] for x in _bytes(rest)] == [x[1:] for x in whole[3:]]
    assert [x[0] for x in _bytes(rest)] == [x[0] for x in _bytes(run[3:])]
    for h in (v, other):
        h.close()


# --------------------------------------------------------------------------------------- the stateless calls
@pytest.mark.parametrize("m", [1, 65, 257])
def test_stateless_calls_at_any_m(m):
    c, big = K.case(1025), K.case(4097)
    v = _of_case(c)
    v.reset(c.reset_obs); v.step(*c.steps[0])
    stats, returns = v.stats(), v.returns()
    ref = R.RefVecNormalize(1025, clip_obs=c.clip_obs, clip_reward=c.clip_reward, gamma=K.GAMMA, epsilon=K.EPSILON)
    ref.reset(c.reset_obs); ref.step(*c.steps[0])
    host = K.HostVecNormalize(1025, clip_obs=c.clip_obs, clip_reward=c.clip_reward)
    host.set_stats(stats)
    x, r = np.ascontiguousarray(big.steps[1][0][:m]), np.ascontiguousarray(big.steps[2][1][:m])   # rows with both outliers among them
    got_x, got_r = v.normalize("obs", x), v.normalize("reward", r)
    K.assert_outputs_close(got_x, ref.normalize_obs(x), c.clip_obs, ("normalize_obs", m))
    K.assert_outputs_close(got_r, ref.normalize_reward(r), c.clip_reward, ("normalize_reward", m))
    print(f"m = {m}: stateless outputs equal the host build's bytes: "
          f"{got_x.tobytes() == host.normalize_obs(x).tobytes() and got_r.tobytes() == host.normalize_reward(r).tobytes()}")
    assert v.stats().tobytes() == stats.tobytes() and v.returns().tobytes() == returns.tobytes()
    L = v.L
    buf = C.c_void_p(v.o.t.data_ptr())
    for call in (L.brs_vecnorm_normalize_obs, L.brs_vecnorm_normalize_reward):
        assert call(v.h, 0, buf, buf, None) == -1 and b"m must be positive" in L.brs_vecnorm_last_error(v.h)
        assert call(v.h, 4, None, buf, None) == -1 and b"null argument" in L.brs_vecnorm_last_error(v.h)
    v.close(); host.close()


# --------------------------------------------------------------------------------------- non-finite observations
@pytest.mark.parametrize("poison", [np.nan, np.inf])
def test_a_non_finite_observation_stays_in_its_column(poison):
    """ordinary floats that happen not to be finite: the column's statistics leave the finite numbers when the reference's
    do (a NaN gives NaN in both; an Inf gives an Inf mean and a NaN variance in the reference and, through Inf - Inf in a
    later merge of the tree, NaN for both on the device: the class is `not finite`), nothing else changes"""
    n, at, env, col = 257, 3, 100, 3
    c = K.case(n)
    steps = [tuple(a.copy() for a in s) for s in c.steps]
    steps[at][0][env, col] = poison
    v, unpoisoned = _of_case(c), _of_case(c)
    clean = _run(unpoisoned, c)
    unpoisoned.close()
    ref = R.RefVecNormalize(n, clip_obs=c.clip_obs, clip_reward=c.clip_reward, gamma=K.GAMMA, epsilon=K.EPSILON)
    v.reset(c.reset_obs); ref.reset(c.reset_obs)
    others = [i for i in range(21) if i not in (col, 6 + col)]   # every mean, variance and count but this column's mean and variance
    keep = [k for k in range(6) if k != col]
    for k, step in enumerate(steps):
        (o, r, t), (ro, rr, rt) = v.step(*step), ref.step(*step)
        stats, want = v.stats(), ref.stats()
        assert np.array_equal(np.isfinite(stats), np.isfinite(want)), (k, stats, want)
        assert np.isfinite(stats[[col, 6 + col]]).all() == (k < at)
        (co, cr, ct), c_stats, c_returns = clean[k + 1]
        assert stats[others].tobytes() == c_stats[others].tobytes() and v.returns().tobytes() == c_returns.tobytes()
        assert o[:, keep].tobytes() == co[:, keep].tobytes() and t[:, keep].tobytes() == ct[:, keep].tobytes() and r.tobytes() == cr.tobytes()
        assert np.array_equal(np.isnan(o), np.isnan(ro)) and np.array_equal(np.isnan(t), np.isnan(rt))
        if k < at:
            assert o.tobytes() == co.tobytes()
        else:
            assert np.isnan(o[:, col]).all()   # a NaN went through the clip as a NaN
    v.close()


# --------------------------------------------------------------------------------------- the Python object
def _flat(sd):
    """a state_dict's statistics in the order of brs_vecnorm_stats"""
    return np.r_[sd["obs_mean"], sd["obs_var"], sd["obs_count"], sd["ret_mean"], sd["ret_var"], sd["ret_count"]].astype(np.float64)


def test_python_object_state_dict_and_checks():
    import torch
    from balance_robot_mujoco_rl_amd import BrsError, DeviceVecNormalize
    n = 257
    c, host = K.case(n), K.host_run(257)
    v = DeviceVecNormalize(n, clip_obs=c.clip_obs, clip_reward=c.clip_reward)
    up = lambda a: torch.tensor(a, device="cuda")
    K.assert_outputs_close(v.reset(up(c.reset_obs)).cpu().numpy(), c.out[0][0], c.clip_obs, "reset")
    for k, step in enumerate(c.steps[:3], 1):
        o, r, t = v.step(*[up(a) for a in step])
        assert o is v.obs and r is v.reward and t is v.terminal_obs
    sd = v.state_dict()
    assert sorted(sd) == sorted(["obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count", "returns"])
    assert _flat(sd).tobytes() == host[3][1].tobytes() and sd["returns"].tobytes() == host[3][2].tobytes()
    w = DeviceVecNormalize(5, training=False, clip_obs=c.clip_obs, clip_reward=c.clip_reward)
    w.load_state_dict(dict(sd, obs_count=sd["obs_count"][0]))   # SB3's scalar count
    assert all(np.array_equal(w.state_dict()[k], sd[k]) for k in sd if k != "returns")
    x = up(np.ascontiguousarray(c.steps[3][0][:5]))
    assert torch.equal(w.normalize_obs(x), v.normalize_obs(up(c.steps[3][0]))[:5])
    assert torch.equal(w.step(x, x[:, 0].contiguous(), torch.zeros(5, dtype=torch.uint8, device="cuda"), torch.zeros(5, dtype=torch.uint8, device="cuda"), x)[0],
                       w.normalize_obs(x))
    for bad in (x.cpu(), x.double(), x[:, :5], torch.zeros((0, 6), device="cuda"), torch.zeros((8, 6), device="cuda")[::2]):
        with pytest.raises(ValueError):
            w.normalize_obs(bad)
    with pytest.raises(ValueError):
        v.step(x, x[:, 0].contiguous(), x[:, 0].contiguous(), x[:, 0].contiguous(), x)
    with pytest.raises(ValueError):
        w.load_state_dict({"obs_mean": sd["obs_mean"]})
    with pytest.raises(BrsError, match="clip_obs must not be negative"):
        DeviceVecNormalize(4, clip_obs=-1.0)
    v.close(); w.close()


# --------------------------------------------------------------------------------------- inside DeviceRollout
def test_device_rollout_with_a_normaliser_against_the_recomputed_rollout():
    """Env01-v1, 256 envs, 8 steps, teacher-forced: the actions of the device run are replayed on a second simulator, and
    the buffer is recomputed from its raw outputs with ref_vecnorm and the policy and GAE references"""
    import torch
    import ref_policy as P
    from offpolicy_cases import gate
    from balance_robot_mujoco_rl_amd import BatchedSim, DeviceVecNormalize, EpisodeMonitor, _lib
    from balance_robot_mujoco_rl_amd.policy import DevicePolicy, DeviceRollout
    n, T, gamma, lam = 256, 8, 0.99, 0.95
    mk = lambda: BatchedSim("Env01-v1", n, device=0, seed=9, auto_reset=True, max_episode_steps=5)
    flat = np.random.default_rng(4).normal(0.0, 0.3, _lib.POLICY_NPARAM).astype(np.float32)
    pol = DevicePolicy(device=0, seed=4)
    pol.set_weights(flat)
    sim, replay, norm, mon, raw_mon = mk(), mk(), DeviceVecNormalize(n, gamma=gamma), EpisodeMonitor(n, max_len=5), EpisodeMonitor(n, max_len=5)
    ro = DeviceRollout(sim, pol, T, gamma=gamma, gae_lambda=lam, monitor=mon, normalize=norm).collect()
    torch.cuda.synchronize()
    ref = R.RefVecNormalize(n, gamma=gamma)
    obs_seq, reward, start = [ref.reset(replay.reset().cpu().numpy())], [], [np.ones(n, np.uint8)]
    booted = 0
    for t in range(T):
        raw = replay.step(ro.action[t].clamp(-1, 1).contiguous())
        raw_mon.update(raw[1], raw[2], raw[3])
        o, r, te, tr, tobs = [a.cpu().numpy() for a in raw]
        no, nr, nt = ref.step(o, r, te, tr, tobs)
        obs_seq.append(no)
        reward.append(P.bootstrap(flat, nt, te, tr, gamma, nr))
        start.append(((te | tr) != 0).astype(np.uint8))
        booted += int(P.bootstrapped(te, tr).sum())
    assert booted > 0, "the sample must hold time limits: the bootstrap reads the normalised terminal observation"
    value = [P.forward(flat, o)[1] for o in obs_seq]
    adv, ret = P.gae(np.array(reward), np.array(value[:T]), np.array(start[:T]), value[T], start[T], gamma, lam)
    gate(ro.obs.cpu().numpy(), np.array(obs_seq[:T]), "rollout obs")
    gate(ro.reward.cpu().numpy(), np.array(reward), "rollout reward")
    gate(ro.value.cpu().numpy(), np.array(value[:T]), "rollout value")
    gate(ro.adv.cpu().numpy(), adv, "rollout adv")
    gate(ro.ret.cpu().numpy(), ret, "rollout ret")
    assert np.array_equal(ro.episode_start.cpu().numpy(), np.array(start[:T]))
    assert R.stat_distance(_flat(norm.state_dict()), ref.stats()) <= K.stat_gate()
    assert mon.stats() == raw_mon.stats() and mon.stats().steps == T   # the monitor saw the env's own reward
    for m in (sim, replay, norm, mon, raw_mon, pol):
        m.close()
