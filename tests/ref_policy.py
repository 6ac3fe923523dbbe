"""The PPO rollout kernels (include/brs_policy.h: brs_policy_act, brs_policy_value, brs_rollout_bootstrap, brs_gae) restated in fp64: what
SB3 does on the host between two env steps of PPO("MlpPolicy") -- ActorCriticPolicy.forward (6-64-64 tanh towers, action_net, value_net,
a diagonal Gaussian with a state-independent log-std), the time-limit bootstrap of collect_rollouts and
RolloutBuffer.compute_returns_and_advantage.  Written from those rules and from the header's description of the random stream, not from
the kernels: the yardstick of tests/test_policy_cases_cpu.py and tests/test_policy_kernels_gpu.py.

  forward    mean [n][2], value [n] from the flat vector of brs_policy.h (ref_learner.unflatten / ref_learner.towers)
  noise      env gid at `step` takes Philox4x32-10(counter = (step, "POLI", gid_lo, gid_hi), key = (seed_lo, seed_hi)); words 0 and 1
             become two 24-bit uniforms in (0, 1) and those one Box-Muller pair (ref_offpolicy.normal_pair)
  act        action = mean + exp(log_std) z; clipped to [-1, 1]; logp = sum(-z^2 / 2 - log_std - log(2 pi) / 2); deterministic: z = 0
  bootstrap  reward + gamma V(terminal_obs) where truncated != 0 and terminated == 0, elsewhere the reward itself
  gae        SB3's recursion, which is test_policy_kernels._ref_gae in fp64"""
import math

import numpy as np
import torch

import ref_learner as RL
import ref_offpolicy as R
from oracle import oracle as O
from test_policy_kernels import _ref_gae

TAG = 0x504f4c49   # "POLI"
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
NPARAM = RL.NPARAM


def log_std_of(flat):
    """the two log-std entries of the flat vector, widened"""
    return np.asarray(flat, np.float64)[NPARAM - 2:]


def forward(flat, obs):
    """-> mean [n][2], value [n] in fp64"""
    with torch.no_grad():
        P = RL.unflatten(torch.from_numpy(np.asarray(flat, np.float64)))
        mean, v = RL.towers(P, torch.from_numpy(np.asarray(obs, np.float64)))
    return mean.numpy(), v.numpy()


def words(seed, gid, step):
    """the four Philox words of every global env index in `gid` (any integers below 2^63, taken as 64-bit) at `step` -> [len(gid)][4]"""
    key = R._key(int(seed))
    out = np.zeros((len(gid), 4), np.uint32)
    for j, g in enumerate(gid):
        g = int(g)
        out[j] = O.philox([int(step) & 0xffffffff, TAG, g & 0xffffffff, (g >> 32) & 0xffffffff], key)
    return out


def noise(seed, env_index_base, step, n):
    """z [n][2] fp64: row i is env env_index_base + i"""
    w = words(seed, [int(env_index_base) + i for i in range(n)], step)
    return np.array([R.normal_pair(int(a), int(b)) for a, b in w[:, :2]]).reshape(n, 2)


def act_from(mean, log_std, z):
    """-> action [n][2], clipped action [n][2], logp [n] in fp64 from given means, log-stds [2] and standard normals"""
    mean, log_std, z = np.asarray(mean, np.float64), np.asarray(log_std, np.float64), np.asarray(z, np.float64)
    action = mean + np.exp(log_std) * z
    logp = (-0.5 * z * z - log_std - HALF_LOG_2PI).sum(axis=1)
    return action, np.clip(action, -1.0, 1.0), logp


def act(flat, obs, seed, env_index_base, step, deterministic=False):
    """-> (action, clipped action, logp, value, z) in fp64"""
    mean, value = forward(flat, obs)
    z = np.zeros((len(obs), 2)) if deterministic else noise(seed, env_index_base, step, len(obs))
    return act_from(mean, log_std_of(flat), z) + (value, z)


def logp_of_action(mean, log_std, action):
    """what the learner recomputes (ref_learner.minibatch_loss): Normal(mean, exp(log_std)).log_prob(action).sum(-1), in fp64"""
    mean, log_std, action = np.asarray(mean, np.float64), np.asarray(log_std, np.float64), np.asarray(action, np.float64)
    u = (action - mean) / np.exp(log_std)
    return (-0.5 * u * u - log_std - HALF_LOG_2PI).sum(axis=1)


def bootstrapped(terminated, truncated):
    """the rows the time-limit bootstrap applies to; any non-zero byte counts as set"""
    return (np.asarray(truncated) != 0) & (np.asarray(terminated) == 0)


def bootstrap(flat, terminal_obs, terminated, truncated, gamma, reward):
    """-> reward [n] fp64.  The value is taken on the bootstrapped rows only: the others' terminal_obs may hold anything"""
    out = np.asarray(reward, np.float64).copy()
    rows = bootstrapped(terminated, truncated)
    if rows.any():
        out[rows] += float(gamma) * forward(flat, np.asarray(terminal_obs)[rows])[1]
    return out


def gae(reward, value, episode_start, last_value, last_done, gamma, lam, dtype=np.float64):
    """-> adv, ret [T][N]; the flags are taken as non-zero / zero"""
    return _ref_gae(np.asarray(reward), np.asarray(value), (np.asarray(episode_start) != 0).astype(np.uint8), np.asarray(last_value),
                    (np.asarray(last_done) != 0).astype(np.uint8), gamma, lam, dtype=dtype)
