"""The DDPG data path (include/brs_policy.h: brs_ddpg_*, brs_replay_*) restated in fp64 numpy: what SB3's
DDPG (TD3 with target_policy_noise = 0 and one critic) does between two gradient steps, with the reference's
net_arch = dict(pi=[300, 200], qf=[200, 150]).  SB3 is not installed here; the rules are the ones the issue of this feature
spells out.  Written from those rules, not from the kernels: the yardstick of tests/test_offpolicy_cpu.py and
tests/test_offpolicy_gpu.py.

  forwards   actor  obs[6] -> 300 -> 200 -> 2, ReLU ReLU tanh;  critic concat(obs, act)[8] -> 200 -> 150 -> 1, ReLU ReLU linear
  act        SB3 _sample_action: mean = actor(obs), or uniform in [-1, 1] during learning_starts; action = clip(mean + sigma z)
  buffer     time-major numpy arrays; next_obs = terminal observation where an episode ended; done = terminated only
  sampling   two independent uniform integers per sample: a row below `size` and an env
Randomness is Philox4x32-10 from the oracle (oracle.philox), blocks as the header documents them."""
import math

import numpy as np

from oracle import oracle as O

OBS, ACT = 6, 2
ACTOR_SIZES, CRITIC_SIZES = (OBS, 300, 200, ACT), (OBS + ACT, 200, 150, 1)
TAG_ACT, TAG_SAMPLE = 0x44445047, 0x5245504c   # "DDPG", "REPL"


def nparam(sizes):
    return sum(o * i + o for i, o in zip(sizes[:-1], sizes[1:]))


NACTOR, NCRITIC = nparam(ACTOR_SIZES), nparam(CRITIC_SIZES)
assert (NACTOR, NCRITIC) == (62702, 32101)


def layers(flat, sizes):
    """flat vector W1 b1 W2 b2 W3 b3 (torch.nn.Linear layout weight[out][in]) -> [(W, b)] in fp64"""
    flat = np.asarray(flat, np.float64)
    assert flat.size == nparam(sizes)
    out, at = [], 0
    for i, o in zip(sizes[:-1], sizes[1:]):
        W = flat[at:at + o * i].reshape(o, i); at += o * i
        b = flat[at:at + o]; at += o
        out.append((W, b))
    return out


def init_params(sizes, rng, scale=1.0):
    """torch.nn.Linear's default init for weight and bias, U(+-1 / sqrt(fan_in)), times `scale`; float32"""
    parts = []
    for i, o in zip(sizes[:-1], sizes[1:]):
        bound = 1.0 / math.sqrt(i)
        parts += [rng.uniform(-bound, bound, size=o * i), rng.uniform(-bound, bound, size=o)]
    return (np.concatenate(parts) * scale).astype(np.float32)


def forward(flat, x, sizes, squash, hidden=False):
    """x [n][sizes[0]] -> [n][sizes[-1]] in fp64; hidden=True also returns the two pre-activations"""
    (W1, b1), (W2, b2), (W3, b3) = layers(flat, sizes)
    x = np.asarray(x, np.float64)
    p1 = x @ W1.T + b1
    p2 = np.maximum(p1, 0.0) @ W2.T + b2
    y = np.maximum(p2, 0.0) @ W3.T + b3
    y = np.tanh(y) if squash else y
    return (y, p1, p2) if hidden else y


def actor(flat, obs, hidden=False):
    return forward(flat, obs, ACTOR_SIZES, True, hidden)


def critic(flat, obs, act, hidden=False):
    x = np.concatenate([np.asarray(obs, np.float64), np.asarray(act, np.float64)], axis=1)
    r = forward(flat, x, CRITIC_SIZES, False, hidden)
    return (r[0][:, 0], r[1], r[2]) if hidden else r[:, 0]


def td_target(actor_t, critic_t, next_obs, reward, done, gamma):
    """y = r + (1 - done) gamma Q'(s', pi'(s')): no target-policy noise, one critic"""
    qn = critic(critic_t, next_obs, actor(actor_t, next_obs))
    return np.asarray(reward, np.float64) + (1.0 - np.asarray(done, np.float64)) * float(gamma) * qn


# ------------------------------------------------------------------------------------------------ randomness
def _key(seed):
    return [seed & 0xffffffff, (seed >> 32) & 0xffffffff]


def act_words(seed, gid, step):
    """the four words of env `gid` (global index) at `step`"""
    return O.philox([step & 0xffffffff, TAG_ACT, gid & 0xffffffff, (gid >> 32) & 0xffffffff], _key(seed))


def normal_pair(w0, w1):
    """Box-Muller on two 24-bit uniforms in (0, 1)"""
    u1, u2 = ((w0 >> 8) + 0.5) / 16777216.0, ((w1 >> 8) + 0.5) / 16777216.0
    r = math.sqrt(-2.0 * math.log(u1))
    return r * math.cos(2.0 * math.pi * u2), r * math.sin(2.0 * math.pi * u2)


def uniform_action(w):
    """the warm-up component of a word: ((w >> 8) - 2^23) / 2^23, in [-1, 1 - 2^-23]"""
    return ((w >> 8) - 8388608) / 8388608.0


def act(actor_flat, obs, seed, env_index_base, step, sigma, random=False):
    """-> (action, mean, noise), each [n][2] fp64"""
    n = len(obs)
    words = [act_words(seed, env_index_base + i, step) for i in range(n)]
    noise = np.array([normal_pair(w[0], w[1]) for w in words])
    mean = np.array([[uniform_action(w[2]), uniform_action(w[3])] for w in words]) if random else actor(actor_flat, obs)
    return np.clip(mean + float(sigma) * noise, -1.0, 1.0), mean, noise


def sample_indices(seed, draw, m, size, n):
    """-> rows [m], envs [m]: sample j takes block (draw, TAG_SAMPLE, j, 0); row = (w0 size) >> 32, env = (w1 n) >> 32"""
    rows, envs = np.zeros(m, np.int32), np.zeros(m, np.int32)
    for j in range(m):
        w = O.philox([draw & 0xffffffff, TAG_SAMPLE, j, 0], _key(seed))
        rows[j], envs[j] = (w[0] * size) >> 32, (w[1] * n) >> 32
    return rows, envs


def index_map(w0, w1, size, n):
    """the map alone, vectorised over uint32 words (the uniformity test feeds it its own words)"""
    w0, w1 = np.asarray(w0, np.uint64), np.asarray(w1, np.uint64)
    return ((w0 * np.uint64(size)) >> np.uint64(32)).astype(np.int64), ((w1 * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


# ------------------------------------------------------------------------------------------------ the buffer
class Buffer:
    """SB3's ReplayBuffer for n envs as plain arrays, time-major, with DeviceReplayBuffer's surface.  The dtypes are the
    storage's (float32 / uint8): the buffer copies, it does not compute, so it is compared byte for byte."""

    def __init__(self, n, cap, fill=0.0, fill_done=0):
        self.n, self.cap, self.pos, self.full = n, cap, 0, False
        f = lambda *s: np.full(s, fill, np.float32)
        self.obs, self.next_obs, self.action, self.reward = f(cap, n, OBS), f(cap, n, OBS), f(cap, n, ACT), f(cap, n)
        self.done = np.full((cap, n), fill_done, np.uint8)

    def arrays(self):
        return self.obs, self.next_obs, self.action, self.reward, self.done

    @property
    def rows(self):
        return self.cap if self.full else self.pos

    def add(self, last_obs, action, obs, terminal_obs, reward, terminated, truncated):
        p = self.pos
        ended = (np.asarray(terminated) != 0) | (np.asarray(truncated) != 0)
        self.obs[p] = last_obs
        self.next_obs[p] = np.where(ended[:, None], terminal_obs, obs)   # the terminal observation, not the reset one
        self.action[p] = action
        self.reward[p] = reward
        timeout = (np.asarray(truncated) != 0) & (np.asarray(terminated) == 0)
        self.done[p] = (ended & ~timeout).astype(np.uint8)               # dones * (1 - timeouts): a time-limit end bootstraps
        self.pos = (p + 1) % self.cap
        self.full = self.full or self.pos == 0

    def gather(self, rows, envs):
        return tuple(a[rows, envs] for a in self.arrays())
