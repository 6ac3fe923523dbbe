"""What the CPU and the GPU tests of VecNormalize share (tests/test_vecnorm_cpu.py, tests/test_vecnorm_gpu.py): seeded streams
of env steps at the edges of the reduction tree, their reference results (tests/ref_vecnorm.py, computed once and never changed),
the gates, and the host build of the kernel source (tests/vecnormhost) behind DeviceVecNormalize's C calls on numpy arrays.

A stream of (n, T): the observations of a reset, then T steps of (obs, reward, terminated, truncated, terminal_obs).
  columns       mean / std of the six observation columns: 0 / 0.1, 10 / 10, -3 / 3, 250 / 0.25 (|mean| / std = 1e3), 0.5 / 2, and
                a constant 7.25; the reward is 1 + 0.2 z (a positive offset, as the envs here pay per step survived)
  outliers      one observation element at +1000 std (step 1) and one at -1000 std (step 2), one reward of -200 (step 2) and, for
                n >= 256, one of +300 (step 0; below, the first rewards lie beyond +clip by themselves and a +300 among so few
                returns would hide the -200): with the clips below something lands beyond each clip at every n
  done flags    terminated with p = 0.1, truncated with p = 0.05, independently (so both occur together); at step 1 every env
                is done, at step 2 none
  terminal_obs  a fresh draw where the env is done, finite junk (1e6 z) elsewhere
  clips         10 and 10 for n >= 256; 1 and 1 below, where a sample of a few values cannot lie 10 of its own standard
                deviations from its own mean
Conditions, decided on the reference alone, the whole stream redrawn where violated (at most ROUNDS times): no normalised value
within 1e-6 (relative) of a clip; an observation element and a reward beyond each clip somewhere in the stream."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import ref_vecnorm as R
from balance_robot_mujoco_rl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_DIR = os.path.join(ROOT, "tests", "vecnormhost")
GXX = ["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I", os.path.join(ROOT, "balance_robot_mujoco_rl_amd", "csrc")]

SIZES = tuple((n, 8) for n in (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)) + ((65537, 3),)   # (n, T); 65,537: 65 partials
GATE = 1e-5             # fp32 outputs: |x - ref| <= GATE max(1, |ref|), offpolicy_cases.GATE
STAT_FLOOR = 1e-13      # the statistics' gate is 64 x (numpy's own distance from the fsum reference), at least this
ROUNDS = 20
COL_MEAN = np.array([0.0, 10.0, -3.0, 250.0, 0.5, 7.25])
COL_STD = np.array([0.1, 10.0, 3.0, 0.25, 2.0, 0.0])
GAMMA, EPSILON = 0.99, 1e-8


def clips(n):
    return (10.0, 10.0) if n >= 256 else (1.0, 1.0)


def _draw(n, T, rng):
    obs_of = lambda: (COL_MEAN + COL_STD * rng.standard_normal((n, 6))).astype(np.float32)
    reset_obs, steps = obs_of(), []
    for t in range(T):
        obs, reward = obs_of(), (1.0 + 0.2 * rng.standard_normal(n)).astype(np.float32)
        te, tr = (rng.random(n) < 0.1).astype(np.uint8), (rng.random(n) < 0.05).astype(np.uint8)
        if t == 1:
            te[:] = 1
        if t == 2:
            te[:], tr[:] = 0, 0
        done = (te | tr) != 0
        tobs = np.where(done[:, None], obs_of(), (1e6 * rng.standard_normal((n, 6))).astype(np.float32)).astype(np.float32)
        e = (7 * t + 3) % n
        if t == 0 and n >= 256:
            reward[e] = 300.0
        if t == 1:
            obs[e, 0] += np.float32(1000 * COL_STD[0])
        if t == 2:
            obs[e, 2] -= np.float32(1000 * COL_STD[2])
            reward[(e + 1) % n] = -200.0
        steps.append((obs, reward, te, tr, tobs))
    return reset_obs, steps


class Case:
    """a stream and what the reference makes of it: after the reset and after every step the outputs, the 21 statistics and
    the returns; `numpy_stats`: the statistics with np.mean / np.var in the place of the exactly rounded sums"""


def _reference(n, reset_obs, steps, moments="fsum", **config):
    ref = R.RefVecNormalize(n, clip_obs=clips(n)[0], clip_reward=clips(n)[1], gamma=GAMMA, epsilon=EPSILON, moments=moments, **config)
    out, stats, returns, z = [(ref.reset(reset_obs),)], [], [], []
    stats.append(ref.stats()); returns.append(ref.returns.copy()); z.append({"obs": ref.last.get("obs")})
    for step in steps:
        out.append(ref.step(*step))
        stats.append(ref.stats()); returns.append(ref.returns.copy()); z.append(dict(ref.last))
    return ref, out, stats, returns, z


def _conditions(n, z):
    """(ok, coverage) of the unclipped float64 values of a reference run"""
    co, cr = clips(n)
    near = False
    cover = dict(obs_hi=False, obs_lo=False, obs_in=False, rew_hi=False, rew_lo=False, rew_in=False)
    for step in z:
        for key, clip, tag in (("obs", co, "obs"), ("terminal_obs", co, None), ("reward", cr, "rew")):
            v = step.get(key)
            if v is None:
                continue
            near |= bool((np.abs(np.abs(v) - clip) <= 1e-6 * clip).any())
            if tag:
                cover[tag + "_hi"] |= bool((v > clip).any()); cover[tag + "_lo"] |= bool((v < -clip).any())
                cover[tag + "_in"] |= bool((np.abs(v) < clip).any())
    return (not near) and all(cover.values()), cover


_CASES = {}


def case(n):
    """the stream of n envs with its reference results; computed once"""
    if n in _CASES:
        return _CASES[n]
    T = dict(SIZES)[n]
    for rounds in range(ROUNDS):
        reset_obs, steps = _draw(n, T, np.random.default_rng(4000 + 97 * n + rounds))
        ref, out, stats, returns, z = _reference(n, reset_obs, steps)
        ok, cover = _conditions(n, z)
        if ok:
            break
    else:
        raise AssertionError(f"n = {n}: no stream met the conditions in {ROUNDS} rounds: {cover}")
    c = Case()
    c.n, c.T, c.reset_obs, c.steps, c.rounds = n, T, reset_obs, steps, rounds
    c.clip_obs, c.clip_reward = clips(n)
    c.out, c.stats, c.returns, c.z = out, stats, returns, z
    c.numpy_stats = _reference(n, reset_obs, steps, moments="numpy")[2]
    # branch coverage of the reference: every end flag combination (where there are enough envs), the all-done and the
    # none-done step, returns cleared and returns kept
    flags = np.concatenate([2 * s[2] + s[3] for s in steps])
    assert n < 63 or set(flags.tolist()) == {0, 1, 2, 3}, (n, set(flags.tolist()))
    assert ((steps[1][2] | steps[1][3]) != 0).all() and not (steps[2][2] | steps[2][3]).any()
    assert (returns[2] == 0).all() and (returns[3] != 0).all()
    for a in [reset_obs] + [x for s in steps for x in s]:
        a.setflags(write=False)
    _CASES[n] = c
    return c


def yardstick():
    """largest distance, over all cases and steps, of numpy's own float64 mean / var from the exactly rounded reference"""
    return max(R.stat_distance(a, b) for n, _ in SIZES for a, b in zip(case(n).numpy_stats, case(n).stats))


def stat_gate():
    return max(64 * yardstick(), STAT_FLOOR)


def assert_outputs_close(got, ref, clip, what):
    """fp32 outputs within GATE of the reference, and the same elements clipped (the cases keep every value 1e-6 away from
    the clips, far more than the outputs' error)"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == np.float32 and got.shape == ref.shape, (what, got.dtype, got.shape)
    err = np.abs(got.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
    assert err.max() <= GATE, (what, float(err.max()))
    for bound in (np.float32(clip), np.float32(-clip)):
        assert np.array_equal(got == bound, ref == bound), (what, "clipped elements differ")
    return float(err.max())


# ------------------------------------------------------------------------------------------------ the host build
def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


_HOST = []


def host_lib():
    """g++ -> libvecnormhost.so in a temporary directory, with its signatures applied; built once per process"""
    if _HOST:
        return _HOST[0]
    so = os.path.join(tempfile.mkdtemp(prefix="vecnormhost"), "libvecnormhost.so")
    subprocess.check_call(GXX + ["-fPIC", "-shared", "-o", so, os.path.join(HOST_DIR, "vecnormhost.cpp")])
    L = C.CDLL(so)
    vp, i = C.c_void_p, C.c_int
    L.vh_create.restype, L.vh_create.argtypes = vp, [i, C.POINTER(_lib.BrsVecnormConfig)]
    for name, args in (("vh_destroy", [vp]), ("vh_reset", [vp, vp, i, vp]), ("vh_step", [vp] * 6 + [i] + [vp] * 3),
                       ("vh_normalize_obs", [vp, i, vp, vp]), ("vh_normalize_reward", [vp, i, vp, vp]), ("vh_get_stats", [vp, vp]),
                       ("vh_set_stats", [vp, vp]), ("vh_get_returns", [vp, vp])):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = None, args
    _HOST.append(L)
    return L


class HostVecNormalize:
    """tests/vecnormhost on numpy arrays; reset / step return fresh arrays"""

    def __init__(self, n, training=True, norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0, gamma=GAMMA, epsilon=EPSILON):
        self.L, self.n, self.training = host_lib(), n, training
        cfg = _lib.BrsVecnormConfig(gamma, epsilon, clip_obs, clip_reward, int(norm_obs), int(norm_reward))
        self.h = C.c_void_p(self.L.vh_create(n, C.byref(cfg)))

    def reset(self, obs):
        out = np.zeros((self.n, 6), np.float32)
        self.L.vh_reset(self.h, _ptr(obs), int(self.training), _ptr(out))
        return out

    def step(self, obs, reward, terminated, truncated, terminal_obs):
        o, r, t = np.zeros((self.n, 6), np.float32), np.zeros(self.n, np.float32), np.zeros((self.n, 6), np.float32)
        self.L.vh_step(self.h, _ptr(obs), _ptr(reward), _ptr(terminated), _ptr(truncated), _ptr(terminal_obs), int(self.training),
                       _ptr(o), _ptr(r), _ptr(t))
        return o, r, t

    def normalize_obs(self, obs):
        out = np.zeros_like(obs)
        self.L.vh_normalize_obs(self.h, len(obs), _ptr(obs), _ptr(out))
        return out

    def normalize_reward(self, reward):
        out = np.zeros_like(reward)
        self.L.vh_normalize_reward(self.h, len(reward), _ptr(reward), _ptr(out))
        return out

    def stats(self):
        s = np.zeros(21, np.float64)
        self.L.vh_get_stats(self.h, _ptr(s))
        return s

    def set_stats(self, s):
        self.L.vh_set_stats(self.h, _ptr(np.ascontiguousarray(s, np.float64)))

    def returns(self):
        r = np.zeros(self.n, np.float64)
        self.L.vh_get_returns(self.h, _ptr(r))
        return r

    def close(self):
        self.L.vh_destroy(self.h)


_HOST_RUNS = {}


def host_run(n):
    """the host build on the stream of case(n): per call (outputs, stats bytes, returns bytes); computed once"""
    if n in _HOST_RUNS:
        return _HOST_RUNS[n]
    c = case(n)
    v = HostVecNormalize(n, clip_obs=c.clip_obs, clip_reward=c.clip_reward)
    run = [((v.reset(c.reset_obs),), v.stats(), v.returns())]
    for step in c.steps:
        run.append((v.step(*step), v.stats(), v.returns()))
    v.close()
    _HOST_RUNS[n] = run
    return run
