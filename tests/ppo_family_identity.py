"""Inputs and runner of tests/test_ppo_family_identity_gpu.py and tools/gen_ppo_family_identity.py: every kernel of the MlpPolicy
path (brs_policy.hip, brs_learner.hip) through the public Python classes, on the case builders the other tests of these kernels
use.  The sha256 of each output's bytes, recorded with one build, is the yardstick for a change that must keep every
floating-point operation with its operands and its order (tests/golden/ppo_family_identity_parent.json).  Test infrastructure.

  rollout/<weights>   n = 257 (four waves plus one row): act sampled with its noise, act deterministic, value alone, the bootstrap
                      on policy_cases' `mixed` flag pattern
  gae                 the GAE_CASES entry (37, 257, .99, .95, .08)
  ppo                 grad at m = 257 on the default grid, at m = 1,000 on two workgroups (two chunks each: the sums live across
                      chunks), the same with two indices out of range, then one apply from the clean m = 1,000 gradient
  a2c                 grad at m = 257 with idx null, at m = 1,000 with an index list on two workgroups, then one apply"""
import hashlib

import numpy as np
import torch

import a2c_cases as AC
import learner_cases as LC
import policy_cases as PC
import ref_a2c as A
import ref_learner as R

N = 257
GAE_CASE = PC.GAE_CASES[1]
GROUPS = tuple(f"rollout/{kind}" for kind in PC.WEIGHT_SETS) + ("gae", "ppo", "a2c")


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


def _info(s):
    """brs_learner_info as LearnerStats hands it back; every float32 is exact in float64"""
    return np.array([s.steps, s.stopped, s.bad_index, s.policy_loss, s.value_loss, s.entropy, s.approx_kl, s.clip_fraction, s.grad_norm_pi,
                     s.grad_norm_vf], np.float64)


def rollout(kind):
    from balance_robot_mujoco_rl_amd.policy import DevicePolicy
    c, b = PC.forward_case(N, kind), PC.bootstrap_case("mixed", N, kind)
    pol = DevicePolicy(device=0, seed=PC.SEED, env_index_base=PC.BASE)
    pol.set_weights(c["params"])
    obs, out = _cuda(c["obs"]), {}
    noise = torch.empty((N, 2), dtype=torch.float32, device="cuda")
    for name, x in zip(("action", "clipped", "logp", "value"), pol.act(obs, PC.STEP, noise=noise)):
        out[f"sampled/{name}"] = _np(x)
    out["sampled/noise"] = _np(noise)
    for name, x in zip(("action", "clipped", "logp", "value"), pol.act(obs, PC.STEP, deterministic=True)):
        out[f"deterministic/{name}"] = _np(x)
    out["value"] = _np(pol.value(obs))
    reward = _cuda(b["reward"])
    pol.bootstrap(_cuda(b["terminal_obs"]), _cuda(b["terminated"]), _cuda(b["truncated"]), PC.GAMMA, reward)
    out["bootstrap/reward"] = _np(reward)
    pol.close()
    return out


def gae():
    from balance_robot_mujoco_rl_amd.policy import gae as device_gae
    c = PC.gae_case(*GAE_CASE)
    adv, ret = device_gae(*[_cuda(c[k]) for k in ("reward", "value", "episode_start", "last_value", "last_done")], c["gamma"], c["lam"])
    return {"adv": _np(adv), "ret": _np(ret)}


def ppo():
    from balance_robot_mujoco_rl_amd import DevicePPOLearner
    cfg, out = R.Cfg(ent_coef=0.01), {}

    def learner(params, max_workgroups):
        lrn = DevicePPOLearner(device=0, lr=cfg.lr, clip_range=cfg.clip_range, vf_coef=cfg.vf_coef, ent_coef=cfg.ent_coef,
                               max_grad_norm=cfg.max_grad_norm_pi, separate_clip=not cfg.joint_norm, max_workgroups=max_workgroups)
        lrn.params.copy_(_cuda(params))
        return lrn

    case, idx = LC.conditioned(257, cfg)
    lrn = learner(case["params"], 0)
    out["m257/grad"] = _np(lrn.grad(*[_cuda(case[k]) for k in ("obs", "act", "logp_old", "adv", "ret")], _cuda(idx.astype(np.int32))))
    lrn.close()
    case, idx = LC.conditioned(1000, cfg)
    dev = [_cuda(case[k]) for k in ("obs", "act", "logp_old", "adv", "ret")]
    lrn = learner(case["params"], 2)
    bad = idx.astype(np.int32).copy()
    bad[5], bad[300] = -1, LC.N_ROWS   # one in each workgroup's share (chunks 0, 2 and 1, 3)
    out["m1000_bad/grad"] = _np(lrn.grad(*dev, _cuda(bad)))
    out["m1000_bad/info"] = _info(lrn.stats())
    out["m1000/grad"] = _np(lrn.grad(*dev, _cuda(idx.astype(np.int32))))
    lrn.apply()
    out.update({"m1000/params": _np(lrn.params), "m1000/m": _np(lrn.m), "m1000/v": _np(lrn.v), "m1000/info": _info(lrn.stats())})
    lrn.close()
    return out


def a2c():
    from balance_robot_mujoco_rl_amd import DeviceA2CLearner
    cfg, out = A.Cfg(ent_coef=0.01, normalize_adv=1), {}

    def learner(params, max_workgroups):
        lrn = DeviceA2CLearner(device=0, lr=cfg.lr, alpha=cfg.alpha, eps=cfg.eps, vf_coef=cfg.vf_coef, ent_coef=cfg.ent_coef,
                               max_grad_norm=cfg.max_grad_norm_pi, normalize_advantage=True, separate_clip=not cfg.joint_norm,
                               max_workgroups=max_workgroups)
        lrn.params.copy_(_cuda(params))
        return lrn

    case, idx = AC.conditioned(257, cfg, whole=True)
    assert idx is None
    lrn = learner(case["params"], 0)
    out["m257_null/grad"] = _np(lrn.grad(*[_cuda(case[k]) for k in A.KEYS]))
    lrn.close()
    case, idx = AC.conditioned(1000, cfg)
    lrn = learner(case["params"], 2)
    out["m1000/grad"] = _np(lrn.grad(*[_cuda(case[k]) for k in A.KEYS], _cuda(idx.astype(np.int32))))
    lrn.apply()
    out.update({"m1000/params": _np(lrn.params), "m1000/sq": _np(lrn.sq), "m1000/info": _info(lrn.stats())})
    lrn.close()
    return out


def run(group):
    """-> {output name: numpy array} of one group of GROUPS"""
    out = rollout(group.split("/")[1]) if group.startswith("rollout/") else {"gae": gae, "ppo": ppo, "a2c": a2c}[group]()
    return {f"{group}/{k}": np.ascontiguousarray(v) for k, v in out.items()}


def digest(a):
    return {"shape": list(a.shape), "dtype": str(a.dtype), "sha256": hashlib.sha256(a.tobytes()).hexdigest()}
