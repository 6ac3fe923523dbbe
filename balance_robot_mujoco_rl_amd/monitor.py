"""Episode statistics on the device (include/brs_policy.h: brs_monitor_*).

The reference wraps its env in SB3's `Monitor` and judges progress with `EvalCallback` -> `evaluate_policy`
(src/sb_rl.py:501, :536-543): the return and the length of every episode.  `EpisodeMonitor` keeps those numbers for all envs
of a BatchedSim in HBM, fed by one kernel per env step that reads the simulator's outputs in place; `evaluate_policy` is
SB3's function of that name on top of it: the same quota of episodes per env, the same mean and standard deviation."""
import ctypes as C
import dataclasses
import math

import numpy as np
import torch

from . import _lib
from ._handle import BrsError, Handle, _need, _p


def episode_count_targets(n_eval_episodes, n_envs):
    """how many episodes of each env count (SB3 evaluate_policy): the quota is spread over the envs, so that envs whose
    episodes end fast cannot fill it"""
    if n_eval_episodes < 0 or n_envs <= 0:
        raise ValueError(f"need n_eval_episodes >= 0 and n_envs > 0, got {n_eval_episodes}, {n_envs}")
    return np.array([(n_eval_episodes + i) // n_envs for i in range(n_envs)], dtype=np.int32)


@dataclasses.dataclass(frozen=True)
class EpisodeStats:
    """brs_episode_stats; the sums run over the counted episodes"""
    episodes: int
    ended: int
    terminated: int
    time_limit: int
    sum_len: int
    sum_len2: int
    steps: int
    sum_ret: float
    sum_ret2: float
    min_ret: float
    max_ret: float
    running_ret: float
    min_len: int
    max_len: int
    first_running: int
    pending: int

    @property
    def mean_ret(self):
        return self.sum_ret / self.episodes if self.episodes else None

    @property
    def std_ret(self):
        """population standard deviation, like np.std"""
        if not self.episodes:
            return None
        m = self.sum_ret / self.episodes
        return math.sqrt(max(0.0, self.sum_ret2 / self.episodes - m * m))

    @property
    def mean_len(self):
        return self.sum_len / self.episodes if self.episodes else None

    @property
    def frac_time_limit(self):
        return self.time_limit / self.episodes if self.episodes else None


def median_from_histogram(hist, lower=False):
    """exact median of the episode lengths a histogram holds: np.median's, the mean of the two middle ones for an even count, or
    with `lower` torch.median's, the lower of the two; None when it is empty or when the median falls among the episodes longer
    than the last bin"""
    hist = np.asarray(hist, dtype=np.int64)
    total = int(hist.sum())
    if total == 0:
        return None
    cum = np.cumsum(hist[1:])   # cum[k - 1] = episodes of length <= k

    def kth(k):   # length of the k-th shortest episode, k from 0
        j = int(np.searchsorted(cum, k + 1))
        return None if j >= cum.size else j + 1
    lo = kth((total - 1) // 2)
    hi = lo if lower else kth(total // 2)
    return None if lo is None or hi is None else 0.5 * (lo + hi)


class EpisodeMonitor(Handle):
    """SB3's Monitor / VecMonitor for the n envs of a BatchedSim, on the device.  update() only enqueues a kernel; stats(),
    histogram() and episodes() wait for the stream and copy a few numbers out."""
    _FAMILY, _WHAT = "brs_monitor", "the episode monitor has"

    def __init__(self, n, device=0, max_len=6000, log_capacity=0):
        self._attach(device)
        self.n, self.max_len, self.log_capacity = int(n), int(max_len), int(log_capacity)
        self._create("brs_monitor_create", self.device.index, self.n, self.max_len, self.log_capacity)
        self._rows = 0

    def reset(self, targets=None):
        """zero everything, running episodes included; `targets`: episodes of each env that count (None: all of them)"""
        tp = None
        if targets is not None:
            targets = np.ascontiguousarray(targets, dtype=np.int32)
            if targets.shape != (self.n,):
                raise ValueError(f"targets: expected {self.n} entries, got shape {targets.shape}")
            tp = targets.ctypes.data_as(C.POINTER(C.c_int32))
        self._check(self.L.brs_monitor_reset(self.h, tp, self._stream()), "brs_monitor_reset")
        self._rows = 0 if targets is None else int(targets.sum())

    def update(self, reward, terminated, truncated):
        """one env step: the three arrays BatchedSim.step returned (float32, uint8, uint8 of n entries, on the device)"""
        n, d = self.n, self.device
        _need(reward, "reward", torch.float32, (n,), d); _need(terminated, "terminated", torch.uint8, (n,), d)
        _need(truncated, "truncated", torch.uint8, (n,), d)
        self._check(self.L.brs_monitor_update(self.h, _p(reward), _p(terminated), _p(truncated), self._stream()), "brs_monitor_update")

    def stats(self):
        s = _lib.BrsEpisodeStats()
        self._check(self.L.brs_monitor_stats(self.h, C.byref(s), self._stream()), "brs_monitor_stats")
        return EpisodeStats(**{k: getattr(s, k) for k, _ in s._fields_})

    def histogram(self):
        """int64 [max_len + 1]: bin k = counted episodes of length k, bin 0 = longer ones"""
        hist = np.zeros(self.max_len + 1, dtype=np.int64)
        self._check(self.L.brs_monitor_histogram(self.h, hist.ctypes.data_as(C.POINTER(C.c_int64)), self._stream()), "brs_monitor_histogram")
        return hist

    def median_len(self, lower=False):
        return median_from_histogram(self.histogram(), lower)

    def episodes(self):
        """the episode log (only with targets): (env int32, return float64, length int32, time_limit uint8), one entry per row;
        a row that is not filled yet has length 0"""
        r = self._rows
        env, ret, ln, tl = np.zeros(r, np.int32), np.zeros(r, np.float64), np.zeros(r, np.int32), np.zeros(r, np.uint8)
        self._check(self.L.brs_monitor_episodes(self.h, env.ctypes.data_as(C.POINTER(C.c_int32)), ret.ctypes.data_as(C.POINTER(C.c_double)),
                                                ln.ctypes.data_as(C.POINTER(C.c_int32)), tl.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                self._stream()), "brs_monitor_episodes")
        return env, ret, ln, tl


def evaluate_policy(act, sim, n_eval_episodes=10, return_episode_rewards=False, poll_every=32, monitor=None):
    """SB3's evaluate_policy on a batched simulator: `act(obs, t) -> actions [n, 2]` is stepped until env i has finished
    (n_eval_episodes + i) // n episodes; the episodes of an env beyond its quota are ignored.

    -> (mean, std) of the episode returns (np.mean / np.std), or (episode_returns, episode_lengths), in the order in which SB3
    appends them: by the step an episode ended on, then by env (the log is kept by env; the counted episodes of an env are its
    first ones, so their lengths add up to the steps they ended on).  The monitor is read every `poll_every` steps; the result
    does not depend on it.  `monitor`: any object with
    EpisodeMonitor's surface (default: a new EpisodeMonitor on the simulator's device)."""
    n = sim.n
    targets = episode_count_targets(n_eval_episodes, n)
    own = monitor is None
    if own:
        monitor = EpisodeMonitor(n, device=sim.device, max_len=max(1, int(sim.max_episode_steps)), log_capacity=int(n_eval_episodes))
    try:
        obs = sim.reset()
        monitor.reset(targets)
        bound = int(targets.max()) * int(sim.max_episode_steps)   # every episode ends at the time limit at the latest
        poll_every = max(1, int(poll_every))
        pending, t = int(monitor.stats().pending), 0
        while pending > 0 and t < bound:
            obs, reward, terminated, truncated, _ = sim.step(act(obs, t))
            monitor.update(reward, terminated, truncated)
            t += 1
            if t % poll_every == 0 or t == bound:
                pending = int(monitor.stats().pending)
        if pending > 0:
            raise BrsError(f"evaluate_policy: {pending} envs have not finished their episodes after {t} steps "
                           f"(max(target) x max_episode_steps): does the simulator reset its envs and have a time limit?")
        env, ret, length, _ = monitor.episodes()
    finally:
        if own:
            monitor.close()
    end = np.cumsum(length, dtype=np.int64)
    first = np.r_[True, env[1:] != env[:-1]] if env.size else np.zeros(0, bool)   # first row of each env
    end -= np.maximum.accumulate(np.where(first, end - length, 0))                # ... minus the steps of the envs before it
    order = np.lexsort((env, end))
    ret, length = ret[order], length[order]
    if return_episode_rewards:
        return ret, length
    return (float(np.mean(ret)), float(np.std(ret))) if ret.size else (float("nan"), float("nan"))
