"""The PPO learner on the device (include/brs_policy.h: brs_learner_*).

The reference calls `model.learn` (src/sb_rl.py:552-556) and SB3's PPO.train() then walks the rollout buffer in minibatches:
actor/critic forward, clipped surrogate + value loss + entropy bonus, backward, clip_grad_norm_, Adam.  On a 9,413-parameter
network that is several dozen launch-bound torch kernels per optimiser step.  `DevicePPOLearner` does one optimiser step in four
HIP kernels (advantage statistics, gradient, reduce, clip + Adam) on the rollout's own tensors; PyTorch owns the parameter vector,
Adam's moments and the stream, and can all-reduce the gradient buffer between grad() and apply().

`DeviceA2CLearner` is SB3's A2C.train() on the same handle: one step on the whole rollout, RMSpropTFLike for Adam."""
import ctypes as C
import dataclasses

import numpy as np
import torch

from . import _lib
from ._handle import Handle, _need, _numpy, _p
from .policy import SB3_LAYOUT

NPARAM, NSTAT = _lib.POLICY_NPARAM, _lib.LEARNER_NSTAT
# tools/train_ppo_torch.py's ActorCritic, in the order of the flat parameter vector (same shapes as SB3_LAYOUT)
TOOL_NAMES = ["pi.0.weight", "pi.0.bias", "pi.2.weight", "pi.2.bias", "pi.4.weight", "pi.4.bias",
              "v.0.weight", "v.0.bias", "v.2.weight", "v.2.bias", "v.4.weight", "v.4.bias", "log_std"]
NAMINGS = {"tool": TOOL_NAMES, "sb3": [name for name, _ in SB3_LAYOUT]}
_SHAPES = [shape for _, shape in SB3_LAYOUT]
_NVF_HEAD = 64 + 1   # the critic's last layer (weight[1][64], bias[1]) sits right before log_std[2]
CRITIC_HEAD = slice(NPARAM - 2 - _NVF_HEAD, NPARAM - 2)


def naming_of(sd):
    for naming, names in NAMINGS.items():
        if names[0] in sd:
            return naming
    raise ValueError("neither tools/train_ppo_torch.py's ActorCritic nor an SB3 MlpPolicy state_dict")


def flatten_state_dict(sd):
    """state_dict in either naming (tensors or arrays) -> (flat float32 array in brs_policy.h order, ret_scale).  The critic is
    taken as it is: in units of `ret_scale` (the tool's buffer of that name; 1 for SB3)"""
    parts = []
    for name, shape in zip(NAMINGS[naming_of(sd)], _SHAPES):
        a = _numpy(sd[name])
        if tuple(a.shape) != shape:
            raise ValueError(f"{name}: expected shape {shape}, got {tuple(a.shape)}")
        parts.append(a.astype(np.float32).ravel())
    rs = sd.get("ret_scale", 1.0)
    return np.concatenate(parts), float(rs.detach().cpu()) if hasattr(rs, "detach") else float(rs)


def unflatten_state_dict(flat, naming="tool", ret_scale=1.0):
    """the inverse: flat tensor or array -> state_dict of torch tensors (copies, on the vector's device)"""
    flat = torch.as_tensor(flat)
    if flat.numel() != NPARAM:
        raise ValueError(f"expected {NPARAM} parameters, got {flat.numel()}")
    sd, off = {}, 0
    for name, shape in zip(NAMINGS[naming], _SHAPES):
        n = int(np.prod(shape))
        sd[name] = flat[off:off + n].detach().clone().reshape(shape); off += n
    if naming == "tool":
        sd["ret_scale"] = torch.tensor(float(ret_scale), device=flat.device)
    elif ret_scale != 1.0:   # SB3's critic predicts returns: fold the unit into its last layer
        sd["value_net.weight"] *= ret_scale; sd["value_net.bias"] *= ret_scale
    return sd


@dataclasses.dataclass(frozen=True)
class LearnerStats:
    """brs_learner_info"""
    steps: int
    stopped: bool
    bad_index: int
    policy_loss: float
    value_loss: float
    entropy: float
    approx_kl: float
    clip_fraction: float
    grad_norm_pi: float
    grad_norm_vf: float


class _DeviceLearner(Handle):
    """what the learners on a brs_learner handle share: the handle, the flat parameter vector and its conversions, the stats"""
    _FAMILY, _WHAT = "brs_learner", "the on-device learner has"

    def _open(self, device, max_workgroups):
        self._attach(device)
        self._create("brs_learner_create", self.device.index, int(max_workgroups))
        self.ret_scale, self.actor_on = 1.0, True
        self.params, self.grad_buf, self._rollout = self._zeros(NPARAM), self._zeros(NPARAM + NSTAT), self._zeros(NPARAM)

    def _zeros(self, n):
        return torch.zeros(n, dtype=torch.float32, device=self.device)

    # ---- parameters
    def load(self, state_dict):
        """ActorCritic (tools/train_ppo_torch.py) or SB3 MlpPolicy weights; the optimiser's state and step count are kept"""
        flat, self.ret_scale = flatten_state_dict(state_dict)
        self.params.copy_(torch.from_numpy(flat))
        return self

    def state_dict(self, naming="tool"):
        return unflatten_state_dict(self.params, naming, self.ret_scale)

    def rollout_params(self):
        """the vector for DevicePolicy.use_device_weights: the critic's last layer times ret_scale, so that brs_policy_act's value
        is in units of the return.  The same tensor on every call, refreshed in place"""
        self._rollout.copy_(self.params)
        if self.ret_scale != 1.0:
            self._rollout[CRITIC_HEAD] *= self.ret_scale
        return self._rollout

    def stats(self):
        """waits for the stream; one small copy"""
        s = _lib.BrsLearnerInfo()
        self._check(self.L.brs_learner_stats(self.h, C.byref(s), self._stream()), "brs_learner_stats")
        return LearnerStats(int(s.steps), bool(s.stopped), int(s.bad_index), *[float(x) for x in s.stat], float(s.grad_norm_pi),
                            float(s.grad_norm_vf))


class DevicePPOLearner(_DeviceLearner):
    """One PPO optimiser step per step(): the minibatch body of SB3's PPO.train().  `separate_clip`: clip actor + log_std and
    critic by norms of their own (tools/train_ppo_torch.py) instead of SB3's single global norm.  `lr`, `ent_coef`, `target_kl`,
    `ret_scale` (the unit of the critic: its target is ret / ret_scale) and `actor_on` (False: critic warm-up, the loss is
    vf_coef x value loss) are plain attributes and may change between steps."""

    def __init__(self, device=0, lr=3e-4, clip_range=0.2, vf_coef=0.5, ent_coef=0.0, max_grad_norm=0.5, separate_clip=False, target_kl=None,
                 normalize_advantage=True, max_workgroups=0, betas=(0.9, 0.999), eps=1e-8):
        self._open(device, max_workgroups)
        self.lr, self.clip_range, self.vf_coef, self.ent_coef = float(lr), float(clip_range), float(vf_coef), float(ent_coef)
        self.max_grad_norm, self.separate_clip, self.target_kl = float(max_grad_norm), bool(separate_clip), target_kl
        self.normalize_advantage, self.betas, self.eps = bool(normalize_advantage), (float(betas[0]), float(betas[1])), float(eps)
        self.m, self.v = self._zeros(NPARAM), self._zeros(NPARAM)

    def config(self):
        kl = self.target_kl
        return _lib.BrsPpoConfig(lr=self.lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, clip_range=self.clip_range,
                                 vf_coef=self.vf_coef, ent_coef=self.ent_coef, max_grad_norm_pi=self.max_grad_norm,
                                 max_grad_norm_vf=self.max_grad_norm, target_kl=0.0 if kl is None else float(kl), ret_scale=float(self.ret_scale),
                                 normalize_adv=int(self.normalize_advantage), actor_on=int(bool(self.actor_on)),
                                 joint_norm=int(not self.separate_clip))

    # ---- one optimiser step
    def begin_iteration(self):
        """clears the early-stop flag: call once per PPO iteration, before its epochs"""
        self._check(self.L.brs_learner_begin_iteration(self.h, self._stream()), "brs_learner_begin_iteration")

    def grad(self, obs, act, logp_old, adv, ret, idx, out=None):
        """the flat rollout (obs [N, 6], act [N, 2], logp_old / adv / ret [N], float32) and the minibatch's rows idx [M] int32 ->
        gradient buffer [NPARAM + NSTAT]: the gradient of the mean loss, then the means of policy loss, value loss, entropy,
        approximate KL and clip fraction.  All-reduce and divide it for data-parallel training, then apply()"""
        d, f32 = self.device, torch.float32
        n, m = obs.shape[0], idx.shape[0]
        _need(obs, "obs", f32, (n, 6), d); _need(act, "act", f32, (n, 2), d); _need(logp_old, "logp_old", f32, (n,), d)
        _need(adv, "adv", f32, (n,), d); _need(ret, "ret", f32, (n,), d); _need(idx, "idx", torch.int32, (m,), d)
        out = self.grad_buf if out is None else _need(out, "grad", f32, (NPARAM + NSTAT,), d)
        cfg = self.config()
        self._check(self.L.brs_learner_grad(self.h, _p(self.params), n, _p(obs), _p(act), _p(logp_old), _p(adv), _p(ret), _p(idx), m,
                                            C.byref(cfg), _p(out), self._stream()), "brs_learner_grad")
        return out

    def apply(self, grad=None):
        """clip_grad_norm_ + one Adam step, unless this iteration was stopped by target_kl"""
        grad = self.grad_buf if grad is None else _need(grad, "grad", torch.float32, (NPARAM + NSTAT,), self.device)
        cfg = self.config()
        self._check(self.L.brs_learner_apply(self.h, _p(self.params), _p(grad), _p(self.m), _p(self.v), C.byref(cfg), self._stream()),
                    "brs_learner_apply")

    def step(self, obs, act, logp_old, adv, ret, idx):
        self.grad(obs, act, logp_old, adv, ret, idx)
        self.apply()


class DeviceA2CLearner(_DeviceLearner):
    """SB3's A2C.train() (include/brs_policy.h: brs_a2c_*): one optimiser step per step() on the whole rollout --
    the gradient of mean(-adv log pi(a | s)) + vf_coef x value loss - ent_coef x entropy, clip_grad_norm_, RMSpropTFLike (`alpha`,
    `eps` inside the root; its state `sq` starts at ONES).  The defaults are SB3's, except that the value loss is the PPO learner's
    0.5 (v - ret / ret_scale)^2: SB3's vf_coef = 0.5 on mse_loss is vf_coef = 1.0 here, and stats().value_loss is 0.5 mean(d^2).
    The returns and advantages are DeviceRollout(n_steps=5, gae_lambda=1.0)'s.  `separate_clip`, `ret_scale`, `actor_on`: as in
    DevicePPOLearner; every setting is a plain attribute and may change between steps."""

    def __init__(self, device=0, lr=7e-4, alpha=0.99, eps=1e-5, vf_coef=1.0, ent_coef=0.0, max_grad_norm=0.5, normalize_advantage=False,
                 separate_clip=False, ret_scale=1.0, actor_on=True, max_workgroups=0):
        self._open(device, max_workgroups)
        self.lr, self.alpha, self.eps, self.vf_coef, self.ent_coef = float(lr), float(alpha), float(eps), float(vf_coef), float(ent_coef)
        self.max_grad_norm, self.normalize_advantage, self.separate_clip = float(max_grad_norm), bool(normalize_advantage), bool(separate_clip)
        self.ret_scale, self.actor_on = float(ret_scale), bool(actor_on)
        self.sq = torch.ones(NPARAM, dtype=torch.float32, device=self.device)

    def config(self):
        return _lib.BrsA2cConfig(lr=self.lr, alpha=self.alpha, eps=self.eps, vf_coef=self.vf_coef, ent_coef=self.ent_coef,
                                 max_grad_norm_pi=self.max_grad_norm, max_grad_norm_vf=self.max_grad_norm, ret_scale=float(self.ret_scale),
                                 normalize_adv=int(self.normalize_advantage), actor_on=int(bool(self.actor_on)),
                                 joint_norm=int(not self.separate_clip))

    def grad(self, obs, act, adv, ret, idx=None, out=None):
        """the flat rollout (obs [N, 6], act [N, 2], adv / ret [N], float32) -> gradient buffer [NPARAM + NSTAT] over all N rows in
        buffer order, or over the rows idx [M] int32: the gradient of the mean loss, then the means of policy loss, value loss
        and entropy and two zeros.  All-reduce and divide it for data-parallel training, then apply()"""
        d, f32 = self.device, torch.float32
        n = obs.shape[0]
        m = n if idx is None else idx.shape[0]
        _need(obs, "obs", f32, (n, 6), d); _need(act, "act", f32, (n, 2), d); _need(adv, "adv", f32, (n,), d); _need(ret, "ret", f32, (n,), d)
        if idx is not None:
            _need(idx, "idx", torch.int32, (m,), d)
        out = self.grad_buf if out is None else _need(out, "grad", f32, (NPARAM + NSTAT,), d)
        cfg = self.config()
        self._check(self.L.brs_a2c_grad(self.h, _p(self.params), n, _p(obs), _p(act), _p(adv), _p(ret), _p(idx), m,
                                        C.byref(cfg), _p(out), self._stream()), "brs_a2c_grad")
        return out

    def apply(self, grad=None):
        """clip_grad_norm_ + one RMSpropTFLike step"""
        grad = self.grad_buf if grad is None else _need(grad, "grad", torch.float32, (NPARAM + NSTAT,), self.device)
        cfg = self.config()
        self._check(self.L.brs_a2c_apply(self.h, _p(self.params), _p(grad), _p(self.sq), C.byref(cfg), self._stream()), "brs_a2c_apply")

    def step(self, obs, act, adv, ret, idx=None):
        self.grad(obs, act, adv, ret, idx)
        self.apply()
