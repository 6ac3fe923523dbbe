"""What the CPU and the GPU tests of the DDPG data path share (tests/test_offpolicy_cpu.py, tests/test_offpolicy_gpu.py): the
case tables, the conditioned inputs (computed once per size and weight set), the env-step streams that exercise every
combination of the two end flags, the gate, and the host build of the kernel source (tests/offpolicyhost) on numpy arrays."""
import ctypes as C
import itertools
import os

import numpy as np

import ref_offpolicy as R
from balance_robot_mujoco_rl_amd import _lib
from hostbuild import GXX, ROOT, _ptr, compile_host  # noqa: F401 (the tests take GXX and ROOT from here)

HOST_DIR = os.path.join(ROOT, "tests", "offpolicyhost")

FORWARD_ROWS = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257)
KERNEL_ROWS = (127, 128, 129)              # the kernel's workgroup edge (4 waves x 32 rows); 31 / 32 / 33 are its wave edge
WEIGHT_SETS = ("init", "x3")               # torch's default init; every weight x 3: tanh saturates, Q is O(10)
GATE = 1e-5                                # |x - ref| <= GATE max(1, |ref|): the project's policy-kernel tolerance
BUFFER_CASES = ((3, 4), (65, 2), (257, 3))  # (n, cap); 2 cap + 1 adds: the buffer wraps twice
SAMPLE_M = (1, 64, 65, 256, 1000)
SEED, GAMMA = 11, 0.99


def weights(kind):
    rng = np.random.default_rng(7)
    scale = {"init": 1.0, "x3": 3.0}[kind]
    return R.init_params(R.ACTOR_SIZES, rng, scale), R.init_params(R.CRITIC_SIZES, rng, scale)


def _active_ok(*pre):
    """per row: between 25 % and 75 % of the (real) units of every given hidden layer are active"""
    ok = np.ones(pre[0].shape[0], bool)
    for p in pre:
        frac = (p > 0).mean(axis=1)
        ok &= (frac >= 0.25) & (frac <= 0.75)
    return ok


_CASES = {}


def conditioned(n, kind):
    """obs [n][6], act [n][2], reward [n], done [n] (float32 / uint8) such that in every hidden layer of actor(obs), critic(obs, act)
    and critic(obs, actor(obs)) -- the three forwards the tests run -- 25 % to 75 % of the units are active: checked on the fp64
    yardstick alone, rows redrawn where violated.  Computed once."""
    key = (n, kind)
    if key in _CASES:
        return _CASES[key]
    actor_w, critic_w = weights(kind)
    rng = np.random.default_rng(1000 + n)
    draw = lambda k: ((rng.standard_normal((k, 6)) * [1.5, 4.0, 0.5, 0.5, 0.5, 0.5]).astype(np.float32),
                      rng.uniform(-1, 1, size=(k, 2)).astype(np.float32))
    obs, act = draw(n)
    for _ in range(200):
        mu, a1, a2 = R.actor(actor_w, obs, hidden=True)
        _, c1, c2 = R.critic(critic_w, obs, act, hidden=True)
        _, t1, t2 = R.critic(critic_w, obs, mu, hidden=True)
        bad = ~_active_ok(a1, a2, c1, c2, t1, t2)
        if not bad.any():
            break
        obs[bad], act[bad] = draw(int(bad.sum()))
    else:
        raise AssertionError("could not condition the inputs")
    reward = rng.standard_normal(n).astype(np.float32)
    done = (np.arange(n) % 3 == 1).astype(np.uint8)
    _CASES[key] = dict(obs=obs, act=act, reward=reward, done=done, actor=actor_w, critic=critic_w)
    return _CASES[key]


def gate(x, ref, what):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    err = np.abs(x - ref) / np.maximum(1.0, np.abs(ref))
    print(f"{what}: largest |x - ref| / max(1, |ref|) = {err.max():.3g}")
    assert err.max() <= GATE, (what, float(err.max()))
    return float(err.max())


def env_steps(n, steps, seed=3):
    """`steps` env steps of n envs as the simulator would return them: per step a dict of last_obs, action, obs, terminal_obs,
    reward, terminated, truncated.  The end flags cycle through all four combinations over envs and steps; every value differs."""
    rng = np.random.default_rng(seed)
    out = []
    combos = list(itertools.product((0, 1), (0, 1)))
    for t in range(steps):
        f32 = lambda *s: rng.standard_normal(s).astype(np.float32)
        flags = np.array([combos[(i + t) % 4] for i in range(n)], np.uint8)
        out.append(dict(last_obs=f32(n, 6), action=f32(n, 2), obs=f32(n, 6), terminal_obs=f32(n, 6), reward=f32(n),
                        terminated=np.ascontiguousarray(flags[:, 0]) * np.uint8(1 + t % 2 * 254),   # "true" is any non-zero byte
                        truncated=np.ascontiguousarray(flags[:, 1])))
    return out


ADD_ORDER = ("last_obs", "action", "obs", "terminal_obs", "reward", "terminated", "truncated")
SENTINEL, SENTINEL_DONE = -7.5, 201


def reference_buffer(n, cap, steps):
    buf = R.Buffer(n, cap, SENTINEL, SENTINEL_DONE)
    for s in steps:
        buf.add(*[s[k] for k in ADD_ORDER])
    return buf


# ------------------------------------------------------------------------------------------------ the host build
def build_host(directory):
    """g++ -> liboffpolicyhost.so in `directory`, with its signatures applied"""
    L = compile_host(directory, "liboffpolicyhost.so", os.path.join(HOST_DIR, "offpolicyhost.cpp"))
    vp, i, st = C.c_void_p, C.c_int, C.POINTER(_lib.BrsReplayStorage)
    L.oh_act.restype, L.oh_act.argtypes = i, [vp, i, vp, C.c_uint64, C.c_int64, C.c_uint32, C.c_float, i, vp, vp, vp]
    L.oh_q.restype, L.oh_q.argtypes = i, [vp, i, vp, vp, vp]
    L.oh_td_target.restype, L.oh_td_target.argtypes = i, [vp, vp, i, vp, vp, vp, C.c_float, vp]
    L.oh_replay_add.restype, L.oh_replay_add.argtypes = i, [st, i, i, i, vp, vp, vp, vp, vp, vp, vp]
    L.oh_replay_sample.restype, L.oh_replay_sample.argtypes = i, [st, i, i, i, i, C.c_uint64, C.c_uint32, st, vp]
    return L


def host_act(L, actor, obs, seed, base, step, sigma, random=False, n=None):
    n = len(obs) if n is None else n
    a, m, z = (np.zeros((n, 2), np.float32) for _ in range(3))
    assert L.oh_act(_ptr(actor), n, _ptr(obs), seed, base, step, sigma, int(random), _ptr(a), _ptr(m), _ptr(z)) == 0
    return a, m, z


def host_q(L, critic, obs, act):
    q = np.zeros(len(obs), np.float32)
    assert L.oh_q(_ptr(critic), len(obs), _ptr(obs), _ptr(act), _ptr(q)) == 0
    return q


def host_td_target(L, actor_t, critic_t, next_obs, reward, done, gamma):
    y = np.zeros(len(next_obs), np.float32)
    assert L.oh_td_target(_ptr(actor_t), _ptr(critic_t), len(next_obs), _ptr(next_obs), _ptr(reward), _ptr(done), gamma, _ptr(y)) == 0
    return y


def storage_of(arrays):
    return _lib.BrsReplayStorage(*[a.ctypes.data for a in arrays])


class HostBuffer:
    """tests/offpolicyhost behind DeviceReplayBuffer's surface, on numpy arrays pre-filled with a sentinel"""

    def __init__(self, L, n, cap, seed=SEED):
        self.L, self.n, self.cap, self.seed = L, n, cap, seed
        b = R.Buffer(n, cap, SENTINEL, SENTINEL_DONE)   # only its arrays are used
        self.arrays = b.arrays()
        self.pos, self.full, self.draw = 0, False, 0

    @property
    def rows(self):
        return self.cap if self.full else self.pos

    def add(self, s):
        st = storage_of(self.arrays)
        assert self.L.oh_replay_add(C.byref(st), self.n, self.cap, self.pos, _ptr(s["last_obs"]), _ptr(s["action"]), _ptr(s["obs"]),
                                    _ptr(s["reward"]), _ptr(s["terminated"]), _ptr(s["truncated"]), _ptr(s["terminal_obs"])) == 0
        self.pos = (self.pos + 1) % self.cap
        self.full = self.full or self.pos == 0

    def sample(self, m, size=None, draw=None):
        out = (np.zeros((m, 6), np.float32), np.zeros((m, 6), np.float32), np.zeros((m, 2), np.float32), np.zeros(m, np.float32), np.zeros(m, np.uint8))
        idx = np.zeros((m, 2), np.int32)
        st, dst = storage_of(self.arrays), storage_of(out)
        d = self.draw if draw is None else draw
        assert self.L.oh_replay_sample(C.byref(st), self.n, self.cap, self.rows if size is None else size, m, self.seed, d, C.byref(dst), _ptr(idx)) == 0
        self.draw += draw is None
        return out, idx
