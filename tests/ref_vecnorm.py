"""numpy fp64 restatement of SB3's RunningMeanStd and VecNormalize, line by line, for the tests of
brs_vecnorm_*.  The mean and the population variance of a batch are taken with math.fsum, i.e. exactly rounded sums: the
yardstick the reduction tree of the kernels is held against.  `moments="numpy"` takes them with np.mean / np.var instead: how
far those two are apart is the unit of the tests' gate."""
import math

import numpy as np


def batch_moments(x, how="fsum"):
    """x [n] or [n][k] float64 -> (mean, population variance) per column"""
    x = np.asarray(x, np.float64)
    if how == "numpy" or not np.isfinite(x).all():   # fsum refuses Inf - Inf; a non-finite batch only has a class, not a value
        with np.errstate(invalid="ignore", over="ignore"):
            return np.mean(x, axis=0), np.var(x, axis=0)
    cols = x.reshape(x.shape[0], -1)
    n = cols.shape[0]
    mean = np.array([math.fsum(cols[:, c]) / n for c in range(cols.shape[1])])
    var = np.array([math.fsum((cols[:, c] - mean[c]) ** 2) / n for c in range(cols.shape[1])])
    return mean.reshape(x.shape[1:]), var.reshape(x.shape[1:])


class RunningMeanStd:
    """stable_baselines3.common.running_mean_std.RunningMeanStd"""

    def __init__(self, epsilon=1e-4, shape=(), moments="fsum"):
        self.mean, self.var, self.count = np.zeros(shape, np.float64), np.ones(shape, np.float64), float(epsilon)
        self.moments = moments

    def update(self, arr):
        batch_mean, batch_var = batch_moments(arr, self.moments)
        self.update_from_moments(batch_mean, batch_var, arr.shape[0])

    def update_from_moments(self, batch_mean, batch_var, batch_count):
        with np.errstate(invalid="ignore", over="ignore"):
            delta = batch_mean - self.mean
            tot_count = self.count + batch_count
            new_mean = self.mean + delta * batch_count / tot_count
            m_a = self.var * self.count
            m_b = batch_var * batch_count
            m_2 = m_a + m_b + np.square(delta) * self.count * batch_count / tot_count
            new_var = m_2 / tot_count
        self.mean, self.var, self.count = new_mean, new_var, tot_count


class RefVecNormalize:
    """stable_baselines3.common.vec_env.VecNormalize over arrays: reset() / step() are reset() / step_wait() with the env's
    outputs passed in.  Outputs are float32, rounded once from the float64 evaluation."""

    def __init__(self, n, training=True, norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8,
                 moments="fsum"):
        self.n, self.training, self.norm_obs, self.norm_reward = n, training, norm_obs, norm_reward
        self.clip_obs, self.clip_reward, self.gamma, self.epsilon = clip_obs, clip_reward, gamma, epsilon
        self.obs_rms, self.ret_rms = RunningMeanStd(shape=(6,), moments=moments), RunningMeanStd(shape=(), moments=moments)
        self.returns = np.zeros(n, np.float64)
        self.last = {}   # the unclipped float64 values of the last call, for the conditions of the cases

    def _obs(self, obs, key):
        if not self.norm_obs:
            return np.array(obs, np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            z = (np.asarray(obs, np.float64) - self.obs_rms.mean) / np.sqrt(self.obs_rms.var + self.epsilon)
        self.last[key] = z
        return np.clip(z, -self.clip_obs, self.clip_obs).astype(np.float32)

    def normalize_obs(self, obs):
        return self._obs(obs, "stateless_obs")

    def normalize_reward(self, reward, key="stateless_reward"):
        if not self.norm_reward:
            return np.array(reward, np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            z = np.asarray(reward, np.float64) / np.sqrt(self.ret_rms.var + self.epsilon)
        self.last[key] = z
        return np.clip(z, -self.clip_reward, self.clip_reward).astype(np.float32)

    def reset(self, obs):
        self.returns = np.zeros(self.n, np.float64)
        if self.training and self.norm_obs:
            self.obs_rms.update(np.asarray(obs, np.float64))
        return self._obs(obs, "obs")

    def step(self, obs, reward, terminated, truncated, terminal_obs):
        if self.training and self.norm_obs:
            self.obs_rms.update(np.asarray(obs, np.float64))
        if self.training:
            self.returns = self.returns * self.gamma + np.asarray(reward, np.float64)
            self.ret_rms.update(self.returns)
        out = self._obs(obs, "obs"), self.normalize_reward(reward, "reward"), self._obs(terminal_obs, "terminal_obs")
        self.returns[(np.asarray(terminated) | np.asarray(truncated)) != 0] = 0.0
        return out

    def stats(self):
        """the 21 doubles in the order of brs_vecnorm_stats"""
        o, r = self.obs_rms, self.ret_rms
        return np.concatenate([o.mean, o.var, np.full(6, o.count), [r.mean, r.var, r.count]]).astype(np.float64)


def stat_distance(got, ref):
    """largest distance of two sets of 21 doubles: means relative to |mean| + sqrt(var), variances to var, counts absolute
    (they are sums of small integers and 1e-4: exact)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    mean = lambda s: np.r_[s[0:6], s[18]]
    var = lambda s: np.r_[s[6:12], s[19]]
    cnt = lambda s: np.r_[s[12:18], s[20]]
    d_mean = np.abs(mean(got) - mean(ref)) / (np.abs(mean(ref)) + np.sqrt(var(ref)))
    d_var = np.abs(var(got) - var(ref)) / var(ref)
    return float(max(d_mean.max(), d_var.max(), np.abs(cnt(got) - cnt(ref)).max()))
