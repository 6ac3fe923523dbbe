"""TD3 (include/brs_policy.h: brs_td3_td_target, brs_ddpg_learner_twin_critic_grad) restated in fp64: SB3's
TD3.train on the reference's DDPG widths.  SB3 is not installed here; the rule is the one the issue of this feature spells out.  Per
gradient step on a minibatch (s, a, r, s', done) of m rows, n_updates counted from 1:

  1. z ~ N(0, 1) per row and action component
  2. eps = clamp(policy_noise z, -noise_clip, +noise_clip)
  3. a' = clamp(pi'(s') + eps, -1, 1)
  4. y = r + (1 - done) gamma min(Q1'(s', a'), Q2'(s', a')), all from the three TARGET networks
  5. Lc = mse(Q1(s, a), y) + mse(Q2(s, a), y), one Adam over the parameters of both critics
  6. only if n_updates % policy_delay == 0: La = -mean Q1(s, pi(s)) through the first, UPDATED critic, Adam on the actor, then the
     Polyak update of the critics' and the actor's targets; on the other steps no target moves

Written from those rules, not from the kernels: the yardstick of tests/test_td3_cpu.py and tests/test_td3_gpu.py.  The target is
numpy on top of ref_offpolicy.py (its Philox, normal_pair, actor and critic); the twin gradient is ref_ddpg_learner.critic_grad per
critic; TorchTD3 is the chained learner, with z taken from the same Philox blocks."""
import numpy as np
import torch

import ref_ddpg_learner as RL
import ref_offpolicy as R
from oracle import oracle as O

NACTOR, NCRITIC, NSTAT = R.NACTOR, R.NCRITIC, 4
TAG_NOISE = 0x5444334e   # "TD3N"


def noise(seed, draw, m):
    """z [m][2] fp64: row j takes Philox4x32-10(counter = (draw, TAG_NOISE, j, 0), key = seed), words 0 and 1 through normal_pair"""
    z = np.zeros((m, 2))
    for j in range(m):
        w = O.philox([draw & 0xffffffff, TAG_NOISE, j, 0], R._key(seed))
        z[j] = R.normal_pair(w[0], w[1])
    return z


def td3_target(actor_t, critics_t, next_obs, reward, done, gamma, policy_noise, noise_clip, seed, draw, parts=False):
    """-> y [m], a' [m][2], z [m][2] in fp64; parts=True: also a dict of what the branches are decided on (the unclipped noise, the
    unclamped action, the two target Q)"""
    m = len(next_obs)
    z = noise(seed, draw, m)
    p = float(policy_noise) * z
    eps = np.clip(p, -float(noise_clip), float(noise_clip))
    raw = R.actor(actor_t, next_obs) + eps
    a = np.clip(raw, -1.0, 1.0)
    q1, q2 = R.critic(critics_t[:NCRITIC], next_obs, a), R.critic(critics_t[NCRITIC:], next_obs, a)
    y = np.asarray(reward, np.float64) + (1.0 - (np.asarray(done) != 0)) * float(gamma) * np.minimum(q1, q2)
    return (y, a, z, dict(p=p, raw=raw, q1=q1, q2=q2)) if parts else (y, a, z)


def twin_critic_grad(critics, obs, act, y, dtype=torch.float64):
    """-> [2 NCRITIC + 4]: d Lc / d critic 0, d Lc / d critic 1 (the gradient of the summed loss w.r.t. one critic is that of its own
    mse), then Lc and mean Q of critic 0, Lc and mean Q of critic 1"""
    g = [RL.critic_grad(critics[k * NCRITIC:(k + 1) * NCRITIC], obs, act, y, dtype) for k in (0, 1)]
    return np.concatenate([g[0][:NCRITIC], g[1][:NCRITIC], g[0][NCRITIC:], g[1][NCRITIC:]])


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


class TorchTD3:
    """the whole update with torch.optim.Adam and lerp_ on flat vectors: actor [NACTOR], critics [2 NCRITIC] and their targets"""

    def __init__(self, actor, critics, dtype=torch.float64, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, tau=0.005, policy_delay=2):
        self.dtype, self.tau, self.policy_delay, self.n_updates = dtype, tau, policy_delay, 0
        self.actor, self.critics = _t(actor, dtype).clone().requires_grad_(True), _t(critics, dtype).clone().requires_grad_(True)
        self.actor_target, self.critics_target = self.actor.detach().clone(), self.critics.detach().clone()
        self.opt_actor = torch.optim.Adam([self.actor], lr=lr, betas=betas, eps=eps)
        self.opt_critics = torch.optim.Adam([self.critics], lr=lr, betas=betas, eps=eps)

    def td3_target(self, next_obs, reward, done, gamma, policy_noise, noise_clip, seed, draw):
        """y from the three target networks in this object's precision (z from the Philox blocks, in fp64 before the cast) -> float32"""
        with torch.no_grad():
            no, z = _t(next_obs, self.dtype), _t(noise(seed, draw, len(next_obs)), self.dtype)
            eps = (policy_noise * z).clamp(-noise_clip, noise_clip)
            a = (RL.net(self.actor_target, no, R.ACTOR_SIZES, True) + eps).clamp(-1.0, 1.0)
            q = torch.minimum(RL.q_of(self.critics_target[:NCRITIC], no, a), RL.q_of(self.critics_target[NCRITIC:], no, a))
            y = _t(reward, self.dtype) + (1.0 - _t(np.asarray(done) != 0, self.dtype)) * gamma * q
        return y.numpy().astype(np.float32)

    def critics_step(self, obs, act, y):
        o, a, yy = _t(obs, self.dtype), _t(act, self.dtype), _t(y, self.dtype)
        self.opt_critics.zero_grad(set_to_none=True)
        loss = sum(((RL.q_of(self.critics[k * NCRITIC:(k + 1) * NCRITIC], o, a) - yy) ** 2).mean() for k in (0, 1))
        loss.backward()
        self.opt_critics.step()

    def actor_step(self, obs):
        o = _t(obs, self.dtype)
        self.opt_actor.zero_grad(set_to_none=True)
        (-RL.q_of(self.critics.detach()[:NCRITIC], o, RL.net(self.actor, o, R.ACTOR_SIZES, True)).mean()).backward()
        self.opt_actor.step()
        with torch.no_grad():
            self.critics_target.lerp_(self.critics, self.tau)
            self.actor_target.lerp_(self.actor, self.tau)

    def step(self, obs, act, y, between=None):
        """-> whether the actor was updated; `between`: called after the critics' step when the actor's pass follows"""
        self.n_updates += 1
        self.critics_step(obs, act, y)
        delayed = self.n_updates % self.policy_delay == 0
        if delayed:
            if between:
                between()
            self.actor_step(obs)
        return delayed

    def flats(self):
        return {k: getattr(self, k).detach().numpy().copy() for k in ("actor", "critics", "actor_target", "critics_target")}
