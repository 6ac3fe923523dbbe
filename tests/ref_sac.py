"""SAC (include/brs_policy.h: brs_sac_*) restated in fp64: SB3's SACPolicy and SAC.train with SB3's defaults on the
reference's DDPG widths (pi=[300, 200], qf=[200, 150]).  SB3 is not installed here; the rule is the one the issue of this feature spells
out.  Per gradient step on a minibatch (s, a, r, s', done) of m rows:

  1. a_pi, logp = actor.action_log_prob(s): mu, log_std = the two heads, log_std = clamp(log_std, -20, 2), u = mu + exp(log_std) z,
     a_pi = tanh(u), logp = Normal(mu, std).log_prob(u).sum - log(1 - a_pi^2 + 1e-6).sum
  2. ent_coef = exp(log_ent_coef).detach(); ent_coef_loss = -(log_ent_coef (logp + target_entropy).detach()).mean(), an Adam step on
     log_ent_coef (with ent_coef="auto"); the VALUE from before that step is used below
  3. a', logp' from the CURRENT actor on s' (SAC has no target actor), y = r + (1 - done) gamma (min(Q1', Q2')(s', a') - ent_coef logp')
     from the two TARGET critics
  4. Lc = 0.5 (mse(Q1(s, a), y) + mse(Q2(s, a), y)), one Adam over both critics
  5. La = mean(ent_coef logp - min(Q1, Q2)(s, a_pi)) through the UPDATED critics, Adam on the actor
  6. the Polyak update of the critics' targets

Written from those rules, not from the kernels: the yardstick of tests/test_sac_cpu.py and tests/test_sac_gpu.py.  The act and the
target are numpy on top of ref_offpolicy.py (its Philox, normal_pair, forward); the gradients are torch autograd on the loss as SB3
writes it (torch.clamp's gradient, 1 - tanh(u)**2 + 1e-6, Normal.log_prob's (u - mu)^2 / (2 std^2)); TorchSAC is the chained learner,
with z taken from the same Philox blocks.  The same code in fp32 measures how far plain fp32 arithmetic is from the yardstick.

The actor VECTOR is [NACTOR + 1]: W1[300][6] b1 W2[200][300] b2 W3[4][200] b3[4] (rows 0-1 of the last layer are actor.mu, rows 2-3
actor.log_std), then log_ent_coef."""
import math

import numpy as np
import torch

import ref_ddpg_learner as RL
import ref_offpolicy as R
from oracle import oracle as O

ACTOR_SIZES = (R.OBS, 300, 200, 2 * R.ACT)
NACTOR, NCRITIC, NSTAT = R.nparam(ACTOR_SIZES), R.NCRITIC, 4
assert NACTOR == 63104
TAG_ACT, TAG_TARGET, TAG_PI = (int.from_bytes(t, "big") for t in (b"SACA", b"SACT", b"SACP"))
LOG_STD_MIN, LOG_STD_MAX, EPS = -20.0, 2.0, 1e-6
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
STATS = ("actor_loss", "mean_logp", "mean_qmin", "ent_coef")


def with_log_ent_coef(actor, log_ent_coef=0.0):
    """the [NACTOR] parameters and a temperature -> the float32 actor vector [NACTOR + 1]"""
    return np.concatenate([np.asarray(actor, np.float32), np.array([log_ent_coef], np.float32)])


def row_noise(tag, seed, draw, m):
    """z [m][2] fp64: row j takes Philox4x32-10(counter = (draw, tag, j, 0), key = seed), words 0 and 1 through normal_pair"""
    z = np.zeros((m, 2))
    for j in range(m):
        w = O.philox([draw & 0xffffffff, tag, j, 0], R._key(seed))
        z[j] = R.normal_pair(w[0], w[1])
    return z


def heads(actor, obs, hidden=False):
    """-> mu [n][2], raw log_std [n][2] (and the two hidden pre-activations) in fp64"""
    r = R.forward(np.asarray(actor)[:NACTOR], obs, ACTOR_SIZES, False, hidden)
    out = r[0] if hidden else r
    return (out[:, :2], out[:, 2:], r[1], r[2]) if hidden else (out[:, :2], out[:, 2:])


def sample(actor, obs, z):
    """-> a [n][2], logp [n] and a dict of what the branches are decided on"""
    mu, raw = heads(actor, obs)
    log_std = np.clip(raw, LOG_STD_MIN, LOG_STD_MAX)
    u = mu + np.exp(log_std) * z
    a = np.tanh(u)
    logp = (-0.5 * z * z - log_std - HALF_LOG_2PI).sum(axis=1) - np.log(1.0 - a * a + EPS).sum(axis=1)
    return a, logp, dict(mu=mu, raw=raw, log_std=log_std, u=u, one_minus_a2=1.0 / np.cosh(u) ** 2)


def act(actor, obs, seed, env_index_base, step, deterministic=False, random=False, n=None):
    """-> (action, mu, log_std (clamped), z), each [n][2] fp64"""
    n = len(obs) if n is None else n
    words = [O.philox([step & 0xffffffff, TAG_ACT, (env_index_base + i) & 0xffffffff, ((env_index_base + i) >> 32) & 0xffffffff], R._key(seed))
             for i in range(n)]
    z = np.array([R.normal_pair(w[0], w[1]) for w in words])
    if random:
        u = np.array([[R.uniform_action(w[2]), R.uniform_action(w[3])] for w in words])
        return u, u.copy(), np.zeros((n, 2)), z
    mu, raw = heads(actor, obs)
    log_std = np.clip(raw, LOG_STD_MIN, LOG_STD_MAX)
    return np.tanh(mu if deterministic else mu + np.exp(log_std) * z), mu, log_std, z


def sac_target(actor, critics_t, next_obs, reward, done, gamma, seed, draw, parts=False):
    """-> y [m], a' [m][2], logp' [m], z [m][2] in fp64; parts=True: also the dict of sample() plus the two target Q"""
    z = row_noise(TAG_TARGET, seed, draw, len(next_obs))
    a, logp, p = sample(actor, next_obs, z)
    q0, q1 = R.critic(critics_t[:NCRITIC], next_obs, a), R.critic(critics_t[NCRITIC:], next_obs, a)
    alpha = math.exp(float(np.asarray(actor)[NACTOR]))   # exp(-inf) = 0: a target without the entropy term
    y = np.asarray(reward, np.float64) + (1.0 - (np.asarray(done) != 0)) * float(gamma) * (np.minimum(q0, q1) - alpha * logp)
    p.update(q0=q0, q1=q1)
    return (y, a, logp, z, p) if parts else (y, a, logp, z)


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def action_log_prob(w, o, z):
    """SB3's actor.action_log_prob on the flat torch vector w [>= NACTOR]: -> a [m][2], logp [m], with the graph"""
    out = RL.net(w[:NACTOR], o, ACTOR_SIZES, False)
    mu, log_std = out[:, :2], torch.clamp(out[:, 2:], LOG_STD_MIN, LOG_STD_MAX)
    std = log_std.exp()
    u = mu + std * z                                                              # rsample
    logp = (-((u - mu) ** 2) / (2.0 * std ** 2) - log_std - HALF_LOG_2PI).sum(dim=1)   # Normal(mu, std).log_prob(u)
    a = torch.tanh(u)
    return a, logp - torch.log(1.0 - a ** 2 + EPS).sum(dim=1)


def min_q(critics, o, a):
    q = torch.stack([RL.q_of(critics[:NCRITIC], o, a), RL.q_of(critics[NCRITIC:], o, a)], dim=1)
    return torch.min(q, dim=1)[0]


def actor_grad(actor, critics, obs, seed, draw, learn_alpha=True, target_entropy=-2.0, dtype=torch.float64):
    """-> [NACTOR + 1 + 4]: d La / d actor, d ent_coef_loss / d log_ent_coef (0 with a fixed ent_coef), then La, mean logp,
    mean min Q and ent_coef"""
    w, c, o = _t(actor, dtype).requires_grad_(True), _t(critics, dtype), _t(obs, dtype)
    z = _t(row_noise(TAG_PI, seed, draw, len(obs)), dtype)
    a, logp = action_log_prob(w, o, z)
    alpha = torch.exp(w[NACTOR].detach())
    qmin = min_q(c, o, a)
    loss = (alpha * logp - qmin).mean()
    total = loss - (w[NACTOR] * (logp + target_entropy).detach()).mean() if learn_alpha else loss
    total.backward()
    return np.concatenate([w.grad.numpy().astype(np.float64), [loss.item(), logp.mean().item(), qmin.mean().item(), alpha.item()]])


def row_terms(actor, critics, obs, seed, draw):
    """the per-row d La / d (actor output) [m][4] in fp64 (their sums are the b3 gradient), and min Q's two candidates [m][2]"""
    f64 = torch.float64
    w, c, o = _t(actor, f64), _t(critics, f64), _t(obs, f64)
    z = _t(row_noise(TAG_PI, seed, draw, len(obs)), f64)
    out = RL.net(w[:NACTOR], o, ACTOR_SIZES, False).detach().requires_grad_(True)
    mu, log_std = out[:, :2], torch.clamp(out[:, 2:], LOG_STD_MIN, LOG_STD_MAX)
    u = mu + log_std.exp() * z
    a = torch.tanh(u)
    logp = (-0.5 * z * z - log_std - HALF_LOG_2PI).sum(dim=1) - torch.log(1.0 - a ** 2 + EPS).sum(dim=1)
    q = torch.stack([RL.q_of(c[:NCRITIC], o, a), RL.q_of(c[NCRITIC:], o, a)], dim=1)
    (torch.exp(w[NACTOR]) * logp - torch.min(q, dim=1)[0]).mean().backward()
    return out.grad.numpy(), q.detach().numpy(), logp.detach().numpy()


def twin_critic_grad(critics, obs, act, y, dtype=torch.float64):
    """-> [2 NCRITIC + 4]: the gradient of Lc = 0.5 (mse(Q1, y) + mse(Q2, y)) w.r.t. critic 0 and critic 1, then the loss share
    0.5 mse and the mean Q of critic 0, and of critic 1"""
    w, o, a, yy = _t(critics, dtype).requires_grad_(True), _t(obs, dtype), _t(act, dtype), _t(y, dtype)
    q = [RL.q_of(w[k * NCRITIC:(k + 1) * NCRITIC], o, a) for k in (0, 1)]
    mse = [((qk - yy) ** 2).mean() for qk in q]
    (0.5 * (mse[0] + mse[1])).backward()
    return np.concatenate([w.grad.numpy().astype(np.float64), [0.5 * mse[0].item(), q[0].mean().item(), 0.5 * mse[1].item(), q[1].mean().item()]])


class TorchSAC:
    """the whole update with torch.optim.Adam and lerp_ in SB3's order: actor [NACTOR] and log_ent_coef as two parameters with an Adam
    each (the same learning rate and defaults), critics [2 NCRITIC] and their target; flats() returns the actor VECTOR [NACTOR + 1]"""

    def __init__(self, actor, critics, dtype=torch.float64, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, tau=0.005, target_entropy=-2.0, learn_alpha=True):
        self.dtype, self.tau, self.target_entropy, self.learn_alpha = dtype, tau, float(target_entropy), learn_alpha
        full = _t(actor, dtype)
        self.pi = full[:NACTOR].clone().requires_grad_(True)
        self.log_ent_coef = full[NACTOR:].clone().requires_grad_(True)     # [1]
        self.critics = _t(critics, dtype).clone().requires_grad_(True)
        self.critics_target = self.critics.detach().clone()
        adam = dict(lr=lr, betas=betas, eps=eps)
        self.opt_pi, self.opt_ent = torch.optim.Adam([self.pi], **adam), torch.optim.Adam([self.log_ent_coef], **adam)
        self.opt_critics = torch.optim.Adam([self.critics], **adam)

    def target(self, next_obs, reward, done, gamma, seed, draw):
        """y from the current actor and the target critics in this object's precision (z in fp64 before the cast) -> float32"""
        with torch.no_grad():
            no, z = _t(next_obs, self.dtype), _t(row_noise(TAG_TARGET, seed, draw, len(next_obs)), self.dtype)
            a, logp = action_log_prob(self.pi, no, z)
            v = min_q(self.critics_target, no, a) - torch.exp(self.log_ent_coef[0]) * logp
            y = _t(reward, self.dtype) + (1.0 - _t(np.asarray(done) != 0, self.dtype)) * gamma * v
        return y.numpy().astype(np.float32)

    def step(self, obs, act, y, seed, draw, between=None):
        """`between`: called after the critics' step, before the actor's pass"""
        o, a_buf, yy = _t(obs, self.dtype), _t(act, self.dtype), _t(y, self.dtype)
        z = _t(row_noise(TAG_PI, seed, draw, len(obs)), self.dtype)
        a_pi, logp = action_log_prob(self.pi, o, z)
        ent_coef = torch.exp(self.log_ent_coef.detach())[0]                 # the value before the temperature's step
        if self.learn_alpha:
            self.opt_ent.zero_grad(set_to_none=True)
            (-(self.log_ent_coef * (logp + self.target_entropy).detach()).mean()).backward()
            self.opt_ent.step()
        self.opt_critics.zero_grad(set_to_none=True)
        (0.5 * sum(((RL.q_of(self.critics[k * NCRITIC:(k + 1) * NCRITIC], o, a_buf) - yy) ** 2).mean() for k in (0, 1))).backward()
        self.opt_critics.step()
        if between:
            between()
        self.opt_pi.zero_grad(set_to_none=True)
        (ent_coef * logp - min_q(self.critics.detach(), o, a_pi)).mean().backward()
        self.opt_pi.step()
        with torch.no_grad():
            self.critics_target.lerp_(self.critics, self.tau)

    def flats(self):
        return {"actor": torch.cat([self.pi.detach(), self.log_ent_coef.detach()]).numpy().copy(), "critics": self.critics.detach().numpy().copy(),
                "critics_target": self.critics_target.numpy().copy()}
