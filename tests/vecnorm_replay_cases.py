"""What the CPU and the GPU tests of the normalising replay sample share (tests/test_vecnorm_replay_cpu.py,
tests/test_vecnorm_replay_gpu.py): buffers of raw transitions built from the streams of tests/vecnorm_cases.py,
the reference of a sample, the conditions the cases meet, and the host build of the kernel source (tests/vecnormreplayhost).

A buffer of n envs, CAP = 8 rows: row t is what DeviceOffPolicyCollector hands to the replay buffer at step t of the stream
`vecnorm_cases.case(n)` -- the last observation (the reset's at t = 0), as next observation the terminal observation where the env
ended and the new observation elsewhere, the raw reward, done = terminated -- and a seeded action in [-1, 1).  The statistics are
the reference's after the last step, the clips the stream's.
The reference of a sample: ref_offpolicy.sample_indices, a gather, then RefVecNormalize.normalize_obs / normalize_reward.
Conditions, decided on the reference alone (asserted by the CPU test):
  * no normalised stored value lies within 1e-6 (relative) of a clip;
  * for the largest m, draw_of(n) is the smallest draw whose sample holds every kind of clipped element the storage holds at all:
    at n = 257 and 1,025 an obs element and a reward beyond each clip and a next_obs element below -clip, one cell each (no
    next_obs element exceeds +clip there, so none is demanded); at n = 63, where the clips are 1, obs and next_obs elements beyond
    each clip and a reward below -clip (no reward of that stream exceeds +clip under the final statistics)."""
import ctypes as C
import os
import tempfile

import numpy as np

import hostbuild
import ref_offpolicy as RO
import ref_vecnorm as RV
import vecnorm_cases as K
from balance_robot_mujoco_rl_amd import _lib

HOST_DIR = os.path.join(K.ROOT, "tests", "vecnormreplayhost")
SIZES = (63, 257, 1025)                 # below one workgroup of the moments kernel, an odd size, more than one slab
CAP = 8
MS = (1, 31, 32, 33, 257, 2049)         # the 8-lane and the 32-samples-per-workgroup edges, more than one workgroup, an odd tail
SEED = 0x5eed0123456789
MAX_DRAW = 1 << 15
NEAR = 1e-6


class Buf:
    """a buffer and what belongs to it: the five storage arrays [CAP][n][...], the 21 statistics, the clips"""


_BUFS = {}


def buffer(n):
    if n in _BUFS:
        return _BUFS[n]
    c = K.case(n)
    assert c.T == CAP
    ref, last = RO.Buffer(n, CAP), c.reset_obs
    action = np.random.default_rng(900 + n).uniform(-1.0, 1.0, (CAP, n, 2)).astype(np.float32)
    for t, (obs, reward, te, tr, tobs) in enumerate(c.steps):
        ref.add(last, action[t], obs, tobs, reward, te, tr)
        last = obs
    b = Buf()
    b.n, b.cap, b.case = n, CAP, c
    b.obs, b.next_obs, b.action, b.reward, b.done = ref.arrays()
    b.stats, b.clip_obs, b.clip_reward = c.stats[-1].copy(), c.clip_obs, c.clip_reward
    for a in ref.arrays() + (b.stats,):
        a.setflags(write=False)
    _BUFS[n] = b
    return b


def ref_normalizer(b, norm_obs=True, norm_reward=True, stats=None):
    """a RefVecNormalize holding the buffer's statistics"""
    s = b.stats if stats is None else stats
    v = RV.RefVecNormalize(b.n, norm_obs=norm_obs, norm_reward=norm_reward, clip_obs=b.clip_obs, clip_reward=b.clip_reward, gamma=K.GAMMA,
                           epsilon=K.EPSILON)
    v.obs_rms.mean, v.obs_rms.var, v.obs_rms.count = s[0:6].copy(), s[6:12].copy(), float(s[12])
    v.ret_rms.mean, v.ret_rms.var, v.ret_rms.count = s[18], s[19], float(s[20])
    return v


class Sample:
    """a reference sample: idx [m][2] int32, the five outputs, and `z`: the unclipped float64 values of obs, next_obs, reward"""


def reference_sample(b, m, draw, size=CAP, norm_obs=True, norm_reward=True, arrays=None):
    rows, envs = RO.sample_indices(SEED, draw, m, size, b.n)
    obs, next_obs, action, reward, done = [a[rows, envs] for a in (arrays or (b.obs, b.next_obs, b.action, b.reward, b.done))]
    v = ref_normalizer(b, norm_obs, norm_reward)
    s = Sample()
    s.idx = np.stack([rows, envs], axis=1).astype(np.int32)
    s.obs = v.normalize_obs(obs); z_obs = v.last.get("stateless_obs")
    s.next_obs = v.normalize_obs(next_obs); z_next = v.last.get("stateless_obs")
    s.reward = v.normalize_reward(reward); z_reward = v.last.get("stateless_reward")
    s.action, s.done = action.copy(), done.copy()
    s.z = (z_obs, z_next, z_reward)
    return s


def outputs(s):
    return s.obs, s.next_obs, s.action, s.reward, s.done


def _stored_z(b):
    """the unclipped float64 normalised values of the whole storage: obs, next_obs, reward"""
    if not hasattr(b, "z"):
        v = ref_normalizer(b)
        v.normalize_obs(b.obs.reshape(-1, 6)); zo = v.last["stateless_obs"]
        v.normalize_obs(b.next_obs.reshape(-1, 6)); zn = v.last["stateless_obs"]
        v.normalize_reward(b.reward.reshape(-1)); zr = v.last["stateless_reward"]
        b.z = (zo, zn, zr)
    return b.z


def stored_margin(b):
    """smallest relative distance of a normalised stored value from a clip, over the whole storage"""
    zo, zn, zr = _stored_z(b)
    return min(float(np.abs(np.abs(zo) - b.clip_obs).min() / b.clip_obs), float(np.abs(np.abs(zn) - b.clip_obs).min() / b.clip_obs),
               float(np.abs(np.abs(zr) - b.clip_reward).min() / b.clip_reward))


def _kinds(b, zo, zn, zr):
    return dict(obs_hi=bool((zo > b.clip_obs).any()), obs_lo=bool((zo < -b.clip_obs).any()), next_hi=bool((zn > b.clip_obs).any()),
                next_lo=bool((zn < -b.clip_obs).any()), rew_hi=bool((zr > b.clip_reward).any()), rew_lo=bool((zr < -b.clip_reward).any()))


def stored_kinds(b):
    """which kinds of clipped element the whole storage holds at all"""
    return _kinds(b, *_stored_z(b))


def coverage(b, s):
    """of the kinds the storage holds, which the sample holds"""
    demanded, got = stored_kinds(b), _kinds(b, *s.z)
    return {k: got[k] for k in demanded if demanded[k]}


def philox_words(draw, j, seed=None):
    """words 0 and 1 of the Philox4x32-10 block (draw, TAG_SAMPLE, j, 0) under the key of `seed`, vectorised over numpy arrays of
    draws and sample numbers.  Only the search below uses it (ref_offpolicy.sample_indices takes one block per call); the CPU test
    holds it against sample_indices"""
    seed = SEED if seed is None else seed
    u = lambda x: np.asarray(x, np.uint64)
    c = [u(draw) & u(0xffffffff), u(RO.TAG_SAMPLE), u(j), u(0)]
    k0, k1, mask = seed & 0xffffffff, (seed >> 32) & 0xffffffff, u(0xffffffff)
    for _ in range(10):
        p0, p1 = u(0xD2511F53) * c[0], u(0xCD9E8D57) * c[2]
        c = [(p1 >> u(32)) ^ c[1] ^ u(k0), p1 & mask, (p0 >> u(32)) ^ c[3] ^ u(k1), p0 & mask]
        k0, k1 = (k0 + 0x9E3779B9) & 0xffffffff, (k1 + 0xBB67AE85) & 0xffffffff
    return c[0], c[1]


def cells_of(draws, m, size, n):
    """[len(draws)][m] flat cell numbers row * n + env of the samples of several draws"""
    w0, w1 = philox_words(np.asarray(draws, np.uint64)[:, None], np.arange(m, dtype=np.uint64)[None, :])
    rows, envs = RO.index_map(w0, w1, size, n)
    return rows * n + envs


_DRAWS = {}


def draw_of(n):
    """the smallest draw whose sample of MS[-1] meets the coverage condition; computed once.  The search runs on cell numbers; the
    draw it finds is confirmed on the reference sample itself"""
    if n not in _DRAWS:
        b = buffer(n)
        zo, zn, zr = _stored_z(b)
        per_cell = {"obs_hi": (zo > b.clip_obs).any(axis=1), "obs_lo": (zo < -b.clip_obs).any(axis=1), "next_hi": (zn > b.clip_obs).any(axis=1),
                    "next_lo": (zn < -b.clip_obs).any(axis=1), "rew_hi": zr > b.clip_reward, "rew_lo": zr < -b.clip_reward}
        demanded = [k for k, v in stored_kinds(b).items() if v]
        found = None
        for first in range(0, MAX_DRAW, 256):
            cells = cells_of(np.arange(first, first + 256), MS[-1], CAP, n)
            ok = np.all([per_cell[k][cells].any(axis=1) for k in demanded], axis=0)
            if ok.any():
                found = first + int(np.argmax(ok))
                break
        assert found is not None, f"n = {n}: no draw below {MAX_DRAW} meets the coverage condition"
        assert all(coverage(b, reference_sample(b, MS[-1], found)).values())
        _DRAWS[n] = found
    return _DRAWS[n]


_REFS = {}


def reference(n, m, **kw):
    """the reference sample of (n, m) at draw_of(n); computed once per setting"""
    key = (n, m) + tuple(sorted(kw.items()))
    if key not in _REFS:
        _REFS[key] = reference_sample(buffer(n), m, draw_of(n), **kw)
    return _REFS[key]


def assert_sample_close(got, s, b, what, norm_obs=True, norm_reward=True):
    """the five outputs of a sample against the reference: the normalised ones under vecnorm_cases.assert_outputs_close (GATE, the
    same elements clipped), everything that is copied byte for byte"""
    o, no, a, r, d = got
    for x, ref, name in ((o, s.obs, "obs"), (no, s.next_obs, "next_obs")):
        if norm_obs:
            K.assert_outputs_close(x, ref, b.clip_obs, (what, name))
        else:
            assert x.tobytes() == ref.tobytes(), (what, name)
    if norm_reward:
        K.assert_outputs_close(r, s.reward, b.clip_reward, (what, "reward"))
    else:
        assert r.tobytes() == s.reward.tobytes(), (what, "reward")
    assert a.tobytes() == s.action.tobytes() and d.tobytes() == s.done.tobytes(), (what, "action / done")


# ------------------------------------------------------------------------------------------------ the host build
_HOST = []


def host_lib():
    """g++ -> libvecnormreplayhost.so in a temporary directory, with its signatures applied; built once per process"""
    if _HOST:
        return _HOST[0]
    L = hostbuild.compile_host(tempfile.mkdtemp(prefix="vecnormreplayhost"), "libvecnormreplayhost.so", os.path.join(HOST_DIR, "vecnormreplayhost.cpp"))
    vp, i = C.c_void_p, C.c_int
    L.vrh_create.restype, L.vrh_create.argtypes = vp, [i, C.POINTER(_lib.BrsVecnormConfig)]
    L.vrh_destroy.restype, L.vrh_destroy.argtypes = None, [vp]
    L.vrh_set_stats.restype, L.vrh_set_stats.argtypes = None, [vp, vp]
    L.vrh_replay_sample.restype = i
    L.vrh_replay_sample.argtypes = [vp, C.POINTER(_lib.BrsReplayStorage), i, i, i, i, C.c_uint64, C.c_uint32, C.POINTER(_lib.BrsReplayStorage), vp]
    _HOST.append(L)
    return L


def _store(arrays):
    return _lib.BrsReplayStorage(*[a.ctypes.data for a in arrays])


def host_sample(b, m, draw, size=CAP, norm_obs=True, norm_reward=True):
    """the host build on the buffer -> (obs, next_obs, action, reward, done), idx"""
    L = host_lib()
    cfg = _lib.BrsVecnormConfig(K.GAMMA, K.EPSILON, b.clip_obs, b.clip_reward, int(norm_obs), int(norm_reward))
    h = C.c_void_p(L.vrh_create(b.n, C.byref(cfg)))
    L.vrh_set_stats(h, b.stats.ctypes.data_as(C.c_void_p))
    f = lambda *s: np.full(s, -12345.0, np.float32)
    out = (f(m, 6), f(m, 6), f(m, 2), f(m), np.full(m, 255, np.uint8))
    idx = np.full((m, 2), -1, np.int32)
    src, dst = _store((b.obs, b.next_obs, b.action, b.reward, b.done)), _store(out)
    rc = L.vrh_replay_sample(h, C.byref(src), b.n, b.cap, size, m, SEED, draw, C.byref(dst), idx.ctypes.data_as(C.c_void_p))
    L.vrh_destroy(h)
    assert rc == 0
    return out, idx


_HOST_RUNS = {}


def host_reference(n, m):
    """the host build's sample of (n, m) at draw_of(n); computed once"""
    if (n, m) not in _HOST_RUNS:
        _HOST_RUNS[(n, m)] = host_sample(buffer(n), m, draw_of(n))
    return _HOST_RUNS[(n, m)]


def write_buffer(b, path, draw):
    """the file vecnormreplayhost_main reads"""
    with open(path, "wb") as f:
        f.write(np.array([b.n, b.cap, draw, 0], np.int32).tobytes()); f.write(np.array([b.clip_obs, b.clip_reward], np.float64).tobytes())
        f.write(b.stats.tobytes())
        for a in (b.obs, b.next_obs, b.action, b.reward, b.done):
            f.write(np.ascontiguousarray(a).tobytes())
