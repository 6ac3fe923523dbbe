"""Independent restatement of the episode monitor of DESIGN.md 7.3 (include/brs_policy.h: brs_monitor_*): plain Python and
numpy, one env at a time, nothing shared with the C++.  `RefMonitor` has EpisodeMonitor's surface on host arrays; the kernels,
their host build and evaluate_policy are compared with it.  Also here: the SB3 rules it is held against (the episode quota and
the counting loop of evaluate_policy) and the seeded synthetic streams the CPU and the GPU tests share."""
import functools
import math
import types

import numpy as np

INT_FIELDS = ("episodes", "ended", "terminated", "time_limit", "sum_len", "sum_len2", "steps", "min_len", "max_len", "first_running", "pending")


def sb3_targets(n_eval_episodes, n_envs):
    """stable_baselines3.common.evaluation.evaluate_policy: episode_count_targets"""
    return np.array([(n_eval_episodes + i) // n_envs for i in range(n_envs)], dtype="int")


class RefMonitor:
    def __init__(self, n, max_len=6000, log_capacity=0):
        self.n, self.max_len, self.log_capacity = n, max_len, log_capacity
        self.reset()

    def reset(self, targets=None):
        n = self.n
        if targets is not None:
            targets = [int(t) for t in targets]
            assert len(targets) == n and min(targets) >= 0 and sum(targets) <= self.log_capacity
        self.targets = targets
        self.ep_ret, self.ep_len = [0.0] * n, [0] * n
        self.ended, self.counted = [0] * n, [0] * n
        self.hist = np.zeros(self.max_len + 1, np.int64)
        self.steps = 0
        self.all_ret, self.all_len = [], []          # of the counted episodes, in the order they were counted
        self.n_terminated = self.n_time_limit = 0
        self.pending = n if targets is None else sum(t > 0 for t in targets)
        rows = 0 if targets is None else sum(targets)
        self.base = None if targets is None else [sum(targets[:i]) for i in range(n)]
        self.log = [np.zeros(rows, np.int32), np.zeros(rows, np.float64), np.zeros(rows, np.int32), np.zeros(rows, np.uint8)]

    def update(self, reward, terminated, truncated):
        reward, terminated, truncated = np.asarray(reward), np.asarray(terminated), np.asarray(truncated)
        assert reward.dtype == np.float32 and reward.shape == terminated.shape == truncated.shape == (self.n,)
        self.steps += 1
        for i in range(self.n):
            self.ep_ret[i] = self.ep_ret[i] + float(reward[i])   # Python floats: fp64, in step order
            self.ep_len[i] += 1
            if not (terminated[i] or truncated[i]):
                continue
            ret, length = self.ep_ret[i], self.ep_len[i]
            self.ep_ret[i], self.ep_len[i] = 0.0, 0
            self.ended[i] += 1
            if self.targets is not None and self.counted[i] >= self.targets[i]:
                continue
            k = self.counted[i]
            self.counted[i] += 1
            self.all_ret.append(ret); self.all_len.append(length)
            time_limit = bool(truncated[i]) and not bool(terminated[i])
            self.n_terminated += bool(terminated[i])
            self.n_time_limit += time_limit
            self.hist[length if length <= self.max_len else 0] += 1
            if self.targets is not None:
                row = self.base[i] + k
                for col, v in zip(self.log, (i, ret, length, time_limit)):
                    col[row] = v
                if self.counted[i] == self.targets[i]:
                    self.pending -= 1

    def stats(self):
        r, l = self.all_ret, self.all_len
        return types.SimpleNamespace(
            episodes=len(r), ended=sum(self.ended), terminated=int(self.n_terminated), time_limit=int(self.n_time_limit),
            sum_len=sum(l), sum_len2=sum(x * x for x in l), steps=self.steps,
            sum_ret=math.fsum(r), sum_ret2=math.fsum(x * x for x in r), min_ret=min(r) if r else 0.0, max_ret=max(r) if r else 0.0,
            running_ret=math.fsum(self.ep_ret), min_len=min(l) if l else 0, max_len=max(l) if l else 0,
            first_running=sum(e == 0 for e in self.ended), pending=self.pending,
            # what the tolerance of a reordered fp64 sum is made of
            abs_ret=math.fsum(abs(x) for x in r), abs_running=math.fsum(abs(x) for x in self.ep_ret))

    def histogram(self):
        return self.hist.copy()

    def median_len(self):
        l = sorted(self.all_len)   # None where a middle one is longer than the histogram reaches
        mid = l[(len(l) - 1) // 2:len(l) // 2 + 1]
        return 0.5 * (mid[0] + mid[-1]) if l and mid[-1] <= self.max_len else None

    def episodes(self):
        return tuple(c.copy() for c in self.log)

    def close(self):
        pass


def assert_stats_equal(got, ref):
    """every integer field, min and max exactly; the three fp64 sums within the bound of a reordered sum of m terms,
    (m - 1) 2^-52 sum|x| <= episodes 2^-52 sum|x| (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4 to first
    order), against math.fsum, which is exact up to one rounding"""
    for k in INT_FIELDS:
        assert getattr(got, k) == getattr(ref, k), (k, getattr(got, k), getattr(ref, k))
    assert got.min_ret == ref.min_ret and got.max_ret == ref.max_ret
    u = 2.0 ** -52
    assert abs(got.sum_ret - ref.sum_ret) <= ref.episodes * u * ref.abs_ret, (got.sum_ret, ref.sum_ret)
    assert abs(got.sum_ret2 - ref.sum_ret2) <= ref.episodes * u * ref.sum_ret2, (got.sum_ret2, ref.sum_ret2)


def assert_monitors_equal(got, ref):
    """a monitor under test against the RefMonitor that saw the same stream"""
    s, r = got.stats(), ref.stats()
    assert_stats_equal(s, r)
    assert abs(s.running_ret - r.running_ret) <= ref.n * 2.0 ** -52 * r.abs_running, (s.running_ret, r.running_ret)
    assert np.array_equal(got.histogram(), ref.histogram())
    for a, b in zip(got.episodes(), ref.episodes()):
        assert a.dtype == b.dtype and np.array_equal(a, b)   # returns: bit for bit the fp64 sum in step order
    assert got.median_len() == ref.median_len()


def synthetic_stream(n, steps=40, seed=0, p_done=0.2):
    """[(reward f32 [n], terminated u8 [n], truncated u8 [n])]: rewards of both signs, every combination of the two flags"""
    rng = np.random.default_rng([seed, n])
    out = []
    for _ in range(steps):
        reward = (rng.standard_normal(n) * rng.choice([1e-3, 1.0, 50.0], n)).astype(np.float32)
        done = rng.random(n) < p_done
        kind = rng.integers(0, 3, n)   # 0: terminated, 1: truncated, 2: both
        out.append((reward, (done & (kind != 1)).astype(np.uint8), (done & (kind != 0)).astype(np.uint8)))
    return out


STREAM_SIZES = (1, 63, 64, 65, 257, 1025)


def target_cases(n):
    """None (every episode counts) and the quotas of n_eval_episodes in {1, n - 1, n, 3 n + 7}"""
    return [None] + [sb3_targets(e, n) for e in sorted({1, n - 1, n, 3 * n + 7}) if e >= 0]


STREAM_MAX_LEN = 12   # some episodes of the 40-step streams are longer: bin 0


@functools.lru_cache(maxsize=None)
def stream_reference(n, case, reset_at=None):
    """the RefMonitor that saw synthetic_stream(n) under target_cases(n)[case] (computed once; do not modify it);
    reset_at: the monitor is reset, with the same targets, before that step"""
    targets = target_cases(n)[case]
    ref = RefMonitor(n, STREAM_MAX_LEN, 0 if targets is None else int(targets.sum()))
    ref.reset(targets)
    for t, step in enumerate(synthetic_stream(n)):
        if t == reset_at:
            ref.reset(targets)
        ref.update(*step)
    return ref


def sb3_evaluate_loop(step, reset, n_envs, n_eval_episodes, max_steps):
    """the counting loop of stable_baselines3.common.evaluation.evaluate_policy (no Monitor wrapper, no callback), line by
    line: `reset() -> obs`, `step(obs, t) -> (obs, rewards, dones)` stand for env.reset, model.predict + env.step.
    -> (episode_rewards, episode_lengths, envs, steps taken)"""
    episode_rewards, episode_lengths, envs = [], [], []
    episode_counts = np.zeros(n_envs, dtype="int")
    episode_count_targets = np.array([(n_eval_episodes + i) // n_envs for i in range(n_envs)], dtype="int")
    current_rewards = np.zeros(n_envs)
    current_lengths = np.zeros(n_envs, dtype="int")
    observations = reset()
    t = 0
    while (episode_counts < episode_count_targets).any():
        assert t < max_steps
        observations, rewards, dones = step(observations, t)
        t += 1
        current_rewards += rewards
        current_lengths += 1
        for i in range(n_envs):
            if episode_counts[i] < episode_count_targets[i]:
                if dones[i]:
                    episode_rewards.append(current_rewards[i])
                    episode_lengths.append(current_lengths[i])
                    envs.append(i)
                    episode_counts[i] += 1
                    current_rewards[i] = 0
                    current_lengths[i] = 0
    return episode_rewards, episode_lengths, envs, t
