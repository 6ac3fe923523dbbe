#!/usr/bin/env python3
"""sha256 of what the float actors, critics and learners return on FINITE inputs, one existing test case per family:
a change that only concerns NaN must leave every line as it is.  Run it on two builds of the library and compare the lines:

    python3 tools/finite_output_hashes.py                                   # the product library
    BRS_HIP_LIB=ab/libbrs_hip_parent.so python3 tools/finite_output_hashes.py   # a side build (tools/ab_build.py)

  act / q / the three targets   n = 257, the `init` weights (offpolicy_cases.conditioned, td3_cases.target_case, sac_cases.act_case /
                                target_case); act at sigma 0.1, the SAC act sampled and deterministic
  the five off-policy gradients m = 257 (ddpg_learner_cases.learner_case, td3_cases.twin_case, sac_cases.grad_case)
  PPO and A2C grad_buf          m = 1,000 (learner_cases.conditioned, a2c_cases.conditioned)
"""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import numpy as np
    import torch
    import a2c_cases as AC, ddpg_learner_cases as DC, learner_cases as LC, offpolicy_cases as OC, ref_a2c as A, ref_learner as PL
    import sac_cases as SC, td3_cases as TC
    from balance_robot_mujoco_rl_amd import (DeviceA2CLearner, DeviceDDPGLearner, DeviceDDPGNets, DevicePPOLearner, DeviceSACLearner, DeviceSACNets,
                                             DeviceTD3Learner, _lib)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    lines = []

    def put(name, *tensors):
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in tensors:
            h.update(t.cpu().numpy().tobytes())
        lines.append(f"{name:28s} {h.hexdigest()}")
    n, m, seed, gamma = 257, 257, OC.SEED, OC.GAMMA
    nets, sacnets = DeviceDDPGNets(device=0, seed=seed), DeviceSACNets(device=0, seed=seed)
    c = OC.conditioned(n, "init")
    actor, critic, obs, act, rew, done = (cu(c[k]) for k in ("actor", "critic", "obs", "act", "reward", "done"))
    mean, noise = torch.empty((n, 2), device="cuda"), torch.empty((n, 2), device="cuda")
    put("brs_ddpg_act", nets.act(actor, obs, 3, 0.1, mean=mean, noise=noise), mean, noise)
    put("brs_ddpg_q", nets.q(critic, obs, act))
    put("brs_ddpg_td_target", nets.td_target(actor, critic, obs, rew, done, gamma))
    t = TC.target_case(n, "init", TC.SB3_NOISE)
    na, z = torch.empty((n, 2), device="cuda"), torch.empty((n, 2), device="cuda")
    put("brs_td3_td_target", nets.td3_target(cu(t["actor"]), cu(t["critics"]), cu(t["next_obs"]), cu(t["reward"]), cu(t["done"]), gamma, *TC.SB3_NOISE, 0,
                                             next_action=na, noise=z), na, z)
    s = SC.act_case(n, "init")
    for det in (False, True):
        mu, ls = torch.empty((n, 2), device="cuda"), torch.empty((n, 2), device="cuda")
        put(f"brs_sac_act deterministic={int(det)}", sacnets.act(cu(s["actor"]), cu(s["obs"]), 0, deterministic=det, mean=mu, log_std=ls), mu, ls)
    s = SC.target_case(n, "init")
    lp = torch.empty(n, device="cuda")
    put("brs_sac_td_target", sacnets.sac_target(cu(s["actor"]), cu(s["critics"]), cu(s["next_obs"]), cu(s["reward"]), cu(s["done"]), gamma, 0,
                                                next_action=na, logp=lp), na, lp)
    c, t, s = DC.learner_case(m, "init"), TC.twin_case(m, "init"), SC.grad_case(m, "init")
    ddpg, td3 = DeviceDDPGLearner(device=0, max_batch=m, **DC.ADAM), DeviceTD3Learner(device=0, max_batch=m, **DC.ADAM)
    sac = DeviceSACLearner(device=0, max_batch=m, seed=seed, **{**SC.SAC_ADAM, "target_entropy": SC.TARGET_ENTROPY})
    put("brs_ddpg_learner_critic_grad", ddpg.critic_grad(cu(c["critic"]), cu(c["obs"]), cu(c["act"]), cu(c["y"])))
    put("brs_ddpg_learner_actor_grad", ddpg.actor_grad(cu(c["actor"]), cu(c["critic"]), cu(c["obs"])))
    put("brs_ddpg_learner_twin_critic_grad", td3.twin_critic_grad(cu(t["critics"]), cu(t["obs"]), cu(t["act"]), cu(t["y"])))
    put("brs_sac_twin_critic_grad", sac.twin_critic_grad(cu(s["critics"]), cu(s["obs"]), cu(s["act"]), cu(s["y"])))
    put("brs_sac_actor_grad", sac.actor_grad(cu(s["actor"]), cu(s["critics"]), cu(s["obs"]), 0))
    cfg = PL.Cfg()
    case, idx = LC.conditioned(1000, cfg)
    ppo = DevicePPOLearner(device=0, lr=cfg.lr, clip_range=cfg.clip_range, vf_coef=cfg.vf_coef, ent_coef=cfg.ent_coef, max_grad_norm=cfg.max_grad_norm_pi,
                           separate_clip=not cfg.joint_norm, normalize_advantage=bool(cfg.normalize_adv))
    ppo.params.copy_(cu(case["params"])); ppo.ret_scale, ppo.actor_on = cfg.ret_scale, True
    put("brs_learner_grad m=1000", ppo.grad(*[cu(case[k]) for k in ("obs", "act", "logp_old", "adv", "ret")], cu(idx)))
    cfg = A.Cfg()
    case, idx = AC.conditioned(1000, cfg)
    a2c = DeviceA2CLearner(device=0, lr=cfg.lr, alpha=cfg.alpha, eps=cfg.eps, vf_coef=cfg.vf_coef, ent_coef=cfg.ent_coef, max_grad_norm=cfg.max_grad_norm_pi,
                           normalize_advantage=bool(cfg.normalize_adv), separate_clip=not cfg.joint_norm, ret_scale=cfg.ret_scale)
    a2c.params.copy_(cu(case["params"]))
    put("brs_a2c_grad m=1000", a2c.grad(*[cu(case[k]) for k in A.KEYS], cu(idx)))
    print(f"library {os.environ.get('BRS_HIP_LIB') or 'balance_robot_mujoco_rl_amd/libbrs_hip.so'} build id {_lib.build_id()}")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
