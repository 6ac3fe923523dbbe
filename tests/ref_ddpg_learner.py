"""The DDPG gradient step (include/brs_policy.h: brs_ddpg_learner_*) restated with torch autograd on the flat
parameter vectors, in fp64 by default: SB3's TD3.train as DDPG uses it (one critic, no delay, no target noise).

  1. Lc = mean_i (Q(s_i, a_i) - y_i)^2, its gradient w.r.t. the critic, an Adam step on the critic
  2. La = -mean_i Q(s_i, pi(s_i)) with the critic ALREADY UPDATED, its gradient w.r.t. the actor only, an Adam step on the actor
  3. target <- target + tau (online - target) for both networks, from the updated online weights

Written from those rules, not from the kernels: the yardstick of tests/test_ddpg_learner_cpu.py and tests/test_ddpg_learner_gpu.py.
The layouts are ref_offpolicy.py's.  The same code in fp32 measures how far plain fp32 arithmetic is from the yardstick."""
import numpy as np
import torch

import ref_offpolicy as R

NACTOR, NCRITIC, NSTAT = R.NACTOR, R.NCRITIC, 2
BLOCKS = ("W1", "b1", "W2", "b2", "W3", "b3")


def block_slices(sizes):
    """{block name: slice of the flat vector}"""
    out, at = {}, 0
    for k, (i, o) in enumerate(zip(sizes[:-1], sizes[1:])):
        out[f"W{k + 1}"] = slice(at, at + o * i); at += o * i
        out[f"b{k + 1}"] = slice(at, at + o); at += o
    return out


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def net(flat, x, sizes, squash, hidden=False):
    """the 3-layer network on a flat torch vector; hidden=True also returns the two pre-activations"""
    pre, at = [], 0
    for k, (i, o) in enumerate(zip(sizes[:-1], sizes[1:])):
        W = flat[at:at + o * i].view(o, i); at += o * i
        b = flat[at:at + o]; at += o
        x = x @ W.T + b
        if k < 2:
            pre.append(x)
            x = torch.relu(x)
    x = torch.tanh(x) if squash else x
    return (x, pre[0], pre[1]) if hidden else x


def q_of(critic, obs, act, hidden=False):
    r = net(critic, torch.cat([obs, act], dim=1), R.CRITIC_SIZES, False, hidden)
    return (r[0][:, 0], r[1], r[2]) if hidden else r[:, 0]


def critic_grad(critic, obs, act, y, dtype=torch.float64):
    """-> [NCRITIC + 2]: d Lc / d critic, Lc, mean Q"""
    w = _t(critic, dtype).requires_grad_(True)
    q = q_of(w, _t(obs, dtype), _t(act, dtype))
    loss = ((q - _t(y, dtype)) ** 2).mean()
    loss.backward()
    return np.concatenate([w.grad.numpy(), [loss.item(), q.mean().item()]])


def actor_grad(actor, critic, obs, dtype=torch.float64):
    """-> [NACTOR + 2]: d La / d actor, La, mean pi(s)^2"""
    w, c, o = _t(actor, dtype).requires_grad_(True), _t(critic, dtype), _t(obs, dtype)
    a = net(w, o, R.ACTOR_SIZES, True)
    loss = -q_of(c, o, a).mean()
    loss.backward()
    return np.concatenate([w.grad.numpy(), [loss.item(), (a.detach() ** 2).mean().item()]])


def row_terms(actor, critic, obs, act, y):
    """the per-row terms (fp64) whose sums are the three b3 gradients: 2 (q - y) / m [m], and d La / d (actor output before the
    tanh) [m][2]"""
    f64 = torch.float64
    o, m = _t(obs, f64), len(obs)
    q = q_of(_t(critic, f64), o, _t(act, f64))
    tq = (2.0 * (q - _t(y, f64)) / m).numpy()
    a = net(_t(actor, f64), o, R.ACTOR_SIZES, True).requires_grad_(True)
    (-q_of(_t(critic, f64), o, a).mean()).backward()
    return tq, (a.grad * (1.0 - a.detach() ** 2)).numpy()


def preactivations(actor, critic, obs, act, dtype=torch.float64):
    """the hidden pre-activations of the three forwards the step runs: actor(obs), critic(obs, act), critic(obs, actor(obs)),
    concatenated per row -> [m][300 + 200 + 200 + 150 + 200 + 150]"""
    with torch.no_grad():
        w, c, o = _t(actor, dtype), _t(critic, dtype), _t(obs, dtype)
        mu, a1, a2 = net(w, o, R.ACTOR_SIZES, True, hidden=True)
        _, c1, c2 = q_of(c, o, _t(act, dtype), hidden=True)
        _, t1, t2 = q_of(c, o, mu, hidden=True)
        return torch.cat([a1, a2, c1, c2, t1, t2], dim=1).numpy()


class TorchDDPG:
    """the whole gradient step with torch.optim.Adam and lerp_ on four flat vectors"""

    def __init__(self, actor, critic, dtype=torch.float64, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, tau=0.005):
        self.dtype, self.tau = dtype, tau
        self.actor, self.critic = _t(actor, dtype).clone().requires_grad_(True), _t(critic, dtype).clone().requires_grad_(True)
        self.actor_target, self.critic_target = self.actor.detach().clone(), self.critic.detach().clone()
        self.opt_actor = torch.optim.Adam([self.actor], lr=lr, betas=betas, eps=eps)
        self.opt_critic = torch.optim.Adam([self.critic], lr=lr, betas=betas, eps=eps)

    def critic_step(self, obs, act, y):
        o, a, yy = _t(obs, self.dtype), _t(act, self.dtype), _t(y, self.dtype)
        self.opt_critic.zero_grad(set_to_none=True)
        ((q_of(self.critic, o, a) - yy) ** 2).mean().backward()
        self.opt_critic.step()

    def actor_step(self, obs):
        o = _t(obs, self.dtype)
        self.opt_actor.zero_grad(set_to_none=True)
        (-q_of(self.critic.detach(), o, net(self.actor, o, R.ACTOR_SIZES, True)).mean()).backward()
        self.opt_actor.step()
        with torch.no_grad():
            self.actor_target.lerp_(self.actor, self.tau)
            self.critic_target.lerp_(self.critic, self.tau)

    def step(self, obs, act, y):
        self.critic_step(obs, act, y)
        self.actor_step(obs)

    def td_target(self, next_obs, reward, done, gamma):
        """y from the two target networks, in this object's precision -> float32 [m]"""
        with torch.no_grad():
            no = _t(next_obs, self.dtype)
            qn = q_of(self.critic_target, no, net(self.actor_target, no, R.ACTOR_SIZES, True))
            y = _t(reward, self.dtype) + (1.0 - _t(done, self.dtype)) * gamma * qn
        return y.numpy().astype(np.float32)

    def flats(self):
        return {k: getattr(self, k).detach().numpy().copy() for k in ("actor", "critic", "actor_target", "critic_target")}


class TorchAdam:
    """torch.optim.Adam plus lerp_ on one vector, fed gradients directly (the apply tests)"""

    def __init__(self, params, dtype=torch.float32, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, tau=0.005):
        self.p = _t(params, dtype).clone().requires_grad_(True)
        self.target = self.p.detach().clone()
        self.opt, self.tau = torch.optim.Adam([self.p], lr=lr, betas=betas, eps=eps), tau

    def apply(self, grad):
        self.p.grad = _t(grad, self.p.dtype).clone()
        self.opt.step()
        with torch.no_grad():
            self.target.lerp_(self.p, self.tau)
