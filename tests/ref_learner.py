"""The yardstick of the PPO learner: the minibatch body of tools/train_ppo_torch.py::train restated in torch on
the flat parameter vector of include/brs_policy.h, in any dtype (fp64 is the reference, fp32 measures what fp32 costs), the
clip + torch.optim.Adam step, the inputs the tests share and the per-block error they gate on."""
import dataclasses

import numpy as np
import torch

from balance_robot_mujoco_rl_amd import _lib

NPARAM, NSTAT = _lib.POLICY_NPARAM, _lib.LEARNER_NSTAT
BLOCKS = [(f"{t}.{n}", s) for t, o in (("pi", 2), ("vf", 1)) for n, s in (("W1", (64, 6)), ("b1", (64,)), ("W2", (64, 64)), ("b2", (64,)),
                                                                          ("W3", (o, 64)), ("b3", (o,)))] + [("log_std", (2,))]
GATE = 1e-5            # per block, |g - g64| / |g64|: tests/test_policy_kernels.py's tolerance for the policy kernels against torch
OBS_SCALE = (0.3, 2.0, 5.0, 5.0, 3.0, 3.0)   # the envs' observation ranges


@dataclasses.dataclass
class Cfg:
    """brs_ppo_config with the tool's settings as defaults"""
    lr: float = 3e-4
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-8
    clip_range: float = 0.2
    vf_coef: float = 0.5
    ent_coef: float = 0.0
    max_grad_norm_pi: float = 0.5
    max_grad_norm_vf: float = 0.5
    target_kl: float = 0.0
    ret_scale: float = 1.0
    normalize_adv: int = 1
    actor_on: int = 1
    joint_norm: int = 0

    def c(self):
        return _lib.BrsPpoConfig(**dataclasses.asdict(self))


def block_slices():
    out, off = {}, 0
    for name, shape in BLOCKS:
        n = int(np.prod(shape))
        out[name] = slice(off, off + n); off += n
    assert off == NPARAM
    return out


def unflatten(flat):
    """flat tensor -> {block name: view of its shape}"""
    return {name: flat[sl].view(shape) for (name, shape), sl in zip(BLOCKS, block_slices().values())}


def towers(P, obs):
    def tower(t):
        h = torch.tanh(obs @ P[t + ".W1"].T + P[t + ".b1"])
        h = torch.tanh(h @ P[t + ".W2"].T + P[t + ".b2"])
        return h @ P[t + ".W3"].T + P[t + ".b3"]
    return tower("pi"), tower("vf").squeeze(-1)


def minibatch_loss(P, obs, act, logp_old, adv, ret, cfg, heads=None):
    """tools/train_ppo_torch.py::train, the body of the minibatch loop -> loss, the five stats, the ratio and the advantage used.
    `heads`: the towers' outputs (mean, v) where the caller wants the gradient with respect to them"""
    mean, v = towers(P, obs) if heads is None else heads
    d = torch.distributions.Normal(mean, P["log_std"].exp())
    logp = d.log_prob(act).sum(-1)
    lr_ = logp - logp_old
    ratio = lr_.exp()
    a_ = adv
    if cfg.normalize_adv:
        a_ = (a_ - a_.mean()) / (a_.std() + 1e-8)
    pl = -torch.min(ratio * a_, ratio.clamp(1 - cfg.clip_range, 1 + cfg.clip_range) * a_).mean()
    vl = 0.5 * (v - ret / cfg.ret_scale).pow(2).mean()
    ent = d.entropy().sum(-1).mean()
    loss = cfg.vf_coef * vl if not cfg.actor_on else pl + cfg.vf_coef * vl - cfg.ent_coef * ent
    kl = ((ratio - 1) - lr_).mean()
    clipfrac = ((ratio - 1).abs() > cfg.clip_range).to(ratio.dtype).mean()
    return loss, torch.stack([pl, vl, ent, kl, clipfrac]).detach(), ratio.detach(), a_.detach()


def grad_buffer(case, idx, cfg, dtype=torch.float64, params=None):
    """the gradient buffer of brs_learner_grad (NPARAM gradient entries, then the stats) by autograd in `dtype`"""
    flat = torch.as_tensor(case["params"] if params is None else params).to(dtype).clone().requires_grad_(True)
    i = torch.as_tensor(np.asarray(idx), dtype=torch.long)
    rows = [torch.as_tensor(case[k]).to(dtype)[i] for k in ("obs", "act", "logp_old", "adv", "ret")]
    loss, stats, _, _ = minibatch_loss(unflatten(flat), *rows, cfg)
    loss.backward()
    return torch.cat([flat.grad, stats]).numpy()


ACTOR_BLOCKS = [n for n, _ in BLOCKS if n.startswith("pi.")] + ["log_std"]
CRITIC_BLOCKS = [n for n, _ in BLOCKS if n.startswith("vf.")]


class TorchLearner:
    """params as 13 leaf tensors under torch.optim.Adam with clip_grad_norm_ as the tool (joint_norm 0) or SB3 (1) applies it"""

    def __init__(self, flat, cfg, dtype=torch.float32):
        flat = torch.as_tensor(flat).to(dtype)
        self.cfg, self.dtype = cfg, dtype
        self.P = {k: v.clone().requires_grad_(True) for k, v in unflatten(flat).items()}
        self.opt = torch.optim.Adam(list(self.P.values()), lr=cfg.lr, betas=(cfg.beta1, cfg.beta2), eps=cfg.eps)

    def flat(self):
        return torch.cat([p.detach().reshape(-1) for p in self.P.values()]).numpy()

    def apply(self, grad):
        """one clip + Adam step from a given gradient vector"""
        g = unflatten(torch.as_tensor(np.asarray(grad[:NPARAM])).to(self.dtype).clone())
        for k, p in self.P.items():
            p.grad = g[k].clone()
        cfg = self.cfg
        if cfg.joint_norm:
            torch.nn.utils.clip_grad_norm_(list(self.P.values()), cfg.max_grad_norm_pi)
        else:
            torch.nn.utils.clip_grad_norm_([self.P[k] for k in ACTOR_BLOCKS], cfg.max_grad_norm_pi)
            torch.nn.utils.clip_grad_norm_([self.P[k] for k in CRITIC_BLOCKS], cfg.max_grad_norm_vf)
        self.opt.step()

    def step(self, case, idx):
        """grad + apply by autograd"""
        i = torch.as_tensor(np.asarray(idx), dtype=torch.long)
        rows = [torch.as_tensor(case[k]).to(self.dtype)[i] for k in ("obs", "act", "logp_old", "adv", "ret")]
        self.opt.zero_grad(set_to_none=True)
        loss, _, _, _ = minibatch_loss(self.P, *rows, self.cfg)
        loss.backward()
        self.apply(torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in self.P.values()]).numpy())


def init_params(rng, log_std=-0.5):
    """torch.nn.Linear's default initialisation (uniform in +-1 / sqrt(fan_in)), float32, flat"""
    parts = []
    for name, shape in BLOCKS[:-1]:
        fan_in = 6 if name.endswith("1") else 64
        parts.append(rng.uniform(-1, 1, size=int(np.prod(shape))) / np.sqrt(fan_in))
    return np.concatenate(parts + [np.full(2, log_std)]).astype(np.float32)


def make_case(n_rows=3000, seed=0, cfg=Cfg()):
    """a flat rollout of n_rows rows, float32: observations scaled like the envs', actions sampled from the policy, logp_old the
    true log-prob plus 0.1 x normal, advantages of a few units and returns around +3 (positive rewards, a critic that has not
    learnt them yet)"""
    rng = np.random.default_rng(seed)
    params = init_params(rng)
    obs = (rng.standard_normal((n_rows, 6)) * np.array(OBS_SCALE)).astype(np.float32)
    P = unflatten(torch.as_tensor(params).double())
    mean, _ = towers(P, torch.as_tensor(obs).double())
    sigma = P["log_std"].exp()
    act = (mean + sigma * torch.as_tensor(rng.standard_normal((n_rows, 2)))).numpy().astype(np.float32)
    logp = torch.distributions.Normal(mean, sigma).log_prob(torch.as_tensor(act).double()).sum(-1).numpy()
    return dict(params=params, obs=obs, act=act, logp_true=logp, logp_old=(logp + 0.1 * rng.standard_normal(n_rows)).astype(np.float32),
                adv=(0.3 + 2.0 * rng.standard_normal(n_rows)).astype(np.float32), ret=(3.0 + rng.standard_normal(n_rows)).astype(np.float32),
                rng=rng, redraws=0)


def well_defined(case, idx, cfg, params=None):
    """the issue's input conditions, in fp64: no sample of the minibatch has its ratio within 1e-4 of 1 +- clip_range or its
    (normalised) advantage within 1e-6 of 0 -- there the clip branch could differ between precisions.  -> rows to redraw"""
    flat = torch.as_tensor(case["params"] if params is None else params).double()
    i = torch.as_tensor(np.asarray(idx), dtype=torch.long)
    rows = [torch.as_tensor(case[k]).double()[i] for k in ("obs", "act", "logp_old", "adv", "ret")]
    with torch.no_grad():
        _, _, ratio, a_ = minibatch_loss(unflatten(flat), *rows, cfg)
    bad = ((ratio - (1 - cfg.clip_range)).abs() < 1e-4) | ((ratio - (1 + cfg.clip_range)).abs() < 1e-4) | (a_.abs() < 1e-6)
    return np.unique(np.asarray(idx)[bad.numpy()])


KAPPA_MAX = 4.0


def output_bias_cancellation(case, idx, cfg, params=None):
    """A third input condition, for the gate itself.  The gate is relative to a block's norm, and the smallest blocks, pi.b3 (two
    entries) and vf.b3 (one), are plain sums over the samples of d loss / d mean and d loss / d value.  When such a sum cancels,
    |g64| is small by the luck of the draw and the ratio measures the draw: with terms t_s that each carry an independent relative
    error u (a few fp32 roundings), the sum's error is about u sqrt(sum t^2), i.e. u x kappa relative to it, kappa = sqrt(sum
    t^2) / |sum t|.  The 6.4e-7 that fp32 torch keeps on well-conditioned inputs -- the figure the gate's factor of 15 is counted
    from -- allows kappa up to about 5 at u = 1.2e-7; with zero-mean returns vf.b3 cancelled to 1 / 564 (m = 64) and 1 / 1,236 (m = 255)
    of sum |t|, and fp32 torch itself showed 4.0e-6 and 1.6e-6 on it.  -> the largest kappa over the three entries, in fp64"""
    flat = torch.as_tensor(case["params"] if params is None else params).double()
    i = torch.as_tensor(np.asarray(idx), dtype=torch.long)
    rows = [torch.as_tensor(case[k]).double()[i] for k in ("obs", "act", "logp_old", "adv", "ret")]
    P = unflatten(flat)
    heads = [h.detach().requires_grad_(True) for h in towers(P, rows[0])]
    minibatch_loss(P, *rows, cfg, heads=heads)[0].backward()
    kappa = 0.0
    for d in (heads[0].grad[:, 0], heads[0].grad[:, 1], heads[1].grad):
        if bool(d.any()):
            kappa = max(kappa, float(d.pow(2).sum().sqrt() / d.sum().abs()))
    return kappa


def condition(case, idx, cfg):
    """redraw logp_old's noise, the advantage and the return of the offending rows until the minibatch is well defined"""
    for _ in range(50):
        rows = well_defined(case, idx, cfg)
        if rows.size == 0:
            if output_bias_cancellation(case, idx, cfg) <= KAPPA_MAX:
                return case
            rows = np.unique(np.asarray(idx))   # the sums over the whole minibatch cancel: draw all of its rows again
        rng = case["rng"]
        case["logp_old"][rows] = (case["logp_true"][rows] + 0.1 * rng.standard_normal(rows.size)).astype(np.float32)
        case["adv"][rows] = (0.3 + 2.0 * rng.standard_normal(rows.size)).astype(np.float32)
        case["ret"][rows] = (3.0 + rng.standard_normal(rows.size)).astype(np.float32)
        case["redraws"] += int(rows.size)
    raise AssertionError("the inputs could not be conditioned")


def make_idx(n_rows, m, seed=1):
    """m rows drawn with replacement (repeats allowed); m > n_rows / 8 guarantees some"""
    return np.random.default_rng(seed + m).integers(0, n_rows, size=m).astype(np.int32)


def block_errors(g, g64):
    """{block: |g - g64| / |g64|}; a block whose reference is zero must be zero bit for bit and reports 0"""
    out = {}
    g, g64 = np.asarray(g, np.float64), np.asarray(g64, np.float64)
    for name, sl in block_slices().items():
        ref = np.linalg.norm(g64[sl])
        if ref == 0.0:
            assert not g[sl].any(), f"{name}: the reference gradient is zero, the learner's is not"
            out[name] = 0.0
        else:
            out[name] = float(np.linalg.norm(g[sl] - g64[sl]) / ref)
    return out


def stats_close(g, g64):
    """the five means behind the gradient: fp32 sums of m terms against fp64"""
    np.testing.assert_allclose(np.asarray(g[NPARAM:], np.float64), np.asarray(g64[NPARAM:], np.float64), rtol=1e-5, atol=1e-6)
