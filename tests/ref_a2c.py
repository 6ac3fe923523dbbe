"""The yardstick of the A2C learner: SB3's A2C.train() restated in torch on the flat parameter vector of
include/brs_policy.h, in any dtype (fp64 is the reference, fp32 measures what fp32 costs), clip_grad_norm_ and SB3's RMSpropTFLike
restated from its definition (SB3 is not a dependency), and the input condition of the tests.  The towers, the blocks and the
per-block error are tests/ref_learner.py's.

Value loss: the learner computes vf_coef x 0.5 (v - ret / ret_scale)^2, the PPO learner's convention, so SB3's vf_coef = 0.5 on
mse_loss is vf_coef = 1.0 here; the value-loss statistic is 0.5 mean(d^2)."""
import dataclasses

import numpy as np
import torch

import ref_learner as R
from balance_robot_mujoco_rl_amd import _lib

NPARAM, NSTAT = R.NPARAM, R.NSTAT
KEYS = ("obs", "act", "adv", "ret")


@dataclasses.dataclass
class Cfg:
    """brs_a2c_config with SB3's A2C defaults (vf_coef in this project's convention)"""
    lr: float = 7e-4
    alpha: float = 0.99
    eps: float = 1e-5
    vf_coef: float = 1.0
    ent_coef: float = 0.0
    max_grad_norm_pi: float = 0.5
    max_grad_norm_vf: float = 0.5
    ret_scale: float = 1.0
    normalize_adv: int = 0
    actor_on: int = 1
    joint_norm: int = 1

    def c(self):
        return _lib.BrsA2cConfig(**dataclasses.asdict(self))


def loss(P, obs, act, adv, ret, cfg, heads=None):
    """A2C.train()'s loss on the rows given -> loss, the five stat slots (policy loss, value loss, entropy, 0, 0)"""
    mean, v = R.towers(P, obs) if heads is None else heads
    d = torch.distributions.Normal(mean, P["log_std"].exp())
    logp = d.log_prob(act).sum(-1)
    a_ = adv
    if cfg.normalize_adv:
        a_ = (a_ - a_.mean()) / (a_.std() + 1e-8)
    pl = -(a_ * logp).mean()
    vl = 0.5 * (v - ret / cfg.ret_scale).pow(2).mean()
    ent = d.entropy().sum(-1).mean()
    total = cfg.vf_coef * vl if not cfg.actor_on else pl + cfg.vf_coef * vl - cfg.ent_coef * ent
    zero = torch.zeros((), dtype=pl.dtype)
    return total, torch.stack([pl, vl, ent, zero, zero]).detach()


def _rows(case, idx, dtype):
    i = slice(None) if idx is None else torch.as_tensor(np.asarray(idx), dtype=torch.long)
    return [torch.as_tensor(case[k]).to(dtype)[i] for k in KEYS]


def grad_buffer(case, idx, cfg, dtype=torch.float64, params=None):
    """the gradient buffer of brs_a2c_grad (NPARAM gradient entries, then the stats) by autograd in `dtype`; idx None: every row"""
    flat = torch.as_tensor(case["params"] if params is None else params).to(dtype).clone().requires_grad_(True)
    total, stats = loss(R.unflatten(flat), *_rows(case, idx, dtype), cfg)
    total.backward()
    return torch.cat([flat.grad, stats]).numpy()


class RmspropTFLike64:
    """SB3's RMSpropTFLike(alpha, eps, weight_decay=0, momentum=0, centered=False) on one flat tensor, in fp64 or fp32:
    square_avg starts as ONES; square_avg = square_avg * alpha + (1 - alpha) g g; avg = sqrt(square_avg + eps), epsilon inside
    the root; p = p - lr (g / avg)"""

    def __init__(self, flat, lr=7e-4, alpha=0.99, eps=1e-5, dtype=torch.float64, square_avg=None):
        self.p = torch.as_tensor(np.asarray(flat)).to(dtype).clone()
        self.sq = torch.ones_like(self.p) if square_avg is None else torch.as_tensor(np.asarray(square_avg)).to(dtype).clone()
        self.lr, self.alpha, self.eps, self.dtype = lr, alpha, eps, dtype

    def step(self, g):
        g = torch.as_tensor(np.asarray(g)).to(self.dtype)
        self.sq.mul_(self.alpha).addcmul_(g, g, value=1 - self.alpha)
        avg = self.sq.add(self.eps).sqrt_()
        self.p.addcdiv_(g, avg, value=-self.lr)


class TorchA2C:
    """autograd gradient, clip_grad_norm_ as SB3 (joint_norm 1: one global norm) or per side (0), RmspropTFLike64"""

    def __init__(self, flat, cfg, dtype=torch.float32):
        self.cfg, self.dtype = cfg, dtype
        self.opt = RmspropTFLike64(flat, cfg.lr, cfg.alpha, cfg.eps, dtype)

    def flat(self):
        return self.opt.p.numpy()

    def apply(self, grad):
        g = torch.as_tensor(np.asarray(grad[:NPARAM])).to(self.dtype).clone()
        sl, cfg = R.block_slices(), self.cfg
        critic = torch.zeros(NPARAM, dtype=torch.bool)
        for name in R.CRITIC_BLOCKS:
            critic[sl[name]] = True
        scale = lambda part, max_norm: torch.clamp(max_norm / (part.norm(2) + 1e-6), max=1.0)   # clip_grad_norm_'s coefficient
        if cfg.joint_norm:
            g = g * scale(g, cfg.max_grad_norm_pi)
        else:
            g = torch.where(critic, g * scale(g[critic], cfg.max_grad_norm_vf), g * scale(g[~critic], cfg.max_grad_norm_pi))
        self.opt.step(g)

    def step(self, case, idx):
        flat = self.opt.p.clone().requires_grad_(True)
        loss(R.unflatten(flat), *_rows(case, idx, self.dtype), self.cfg)[0].backward()
        self.apply(flat.grad.numpy())


KAPPA_MAX = 4.0


def kappa(case, idx, cfg):
    """the input condition (DESIGN.md 7.4's rule for the gate's smallest blocks): pi.b3 and vf.b3 are plain sums over the samples
    of d loss / d mean and d loss / d value; kappa = sqrt(sum t^2) / |sum t| of those sums, the largest over the three entries, fp64"""
    flat = torch.as_tensor(case["params"]).double()
    rows = _rows(case, idx, torch.float64)
    P = R.unflatten(flat)
    heads = [h.detach().requires_grad_(True) for h in R.towers(P, rows[0])]
    loss(P, *rows, cfg, heads=heads)[0].backward()
    k = 0.0
    actor = heads[0].grad   # None with actor_on = 0: the loss does not reach the actor
    for d in ([] if actor is None else [actor[:, 0], actor[:, 1]]) + [heads[1].grad]:
        if bool(d.any()):
            k = max(k, float(d.pow(2).sum().sqrt() / d.sum().abs()))
    return k
