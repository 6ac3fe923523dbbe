#!/usr/bin/env python3
"""On-device A2C on the batched simulator: what the reference's `--algorithm A2C` builds, SB3's
A2C('MlpPolicy', env) with its defaults (src/sb_rl.py:72-83) -- five env steps, n-step returns (GAE at lambda = 1), ONE gradient
step over all n_steps x envs rows, clip_grad_norm_(0.5), RMSpropTFLike.  The rollout is DeviceRollout's (act, step, bootstrap and
GAE as HIP kernels); the update is taken in torch, or with --device-learner by DeviceA2CLearner (brs_a2c_*).

    python tools/train_a2c_torch.py --env Env01-v2 --envs 16384 --iters 2000 [--device-learner] [--eval-steps 600] [--out log.json]

The value loss is the PPO tool's 0.5 (v - ret / ret_scale)^2, so --vf-coef 1.0 (the default) is SB3's vf_coef = 0.5 on mse_loss."""
import argparse, json, os, sys, time
import numpy as np
import torch
import torch.distributed as dist
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from train_ppo_torch import ActorCritic, EvalCallback, _allreduce_mean_, allreduce_mean_grads, evaluate, flat_params  # noqa: E402, F401
from balance_robot_mujoco_rl_amd import BatchedSim, EpisodeMonitor  # noqa: E402


class RMSpropTFLike(torch.optim.Optimizer):
    """SB3's RMSpropTFLike without momentum, centering and weight decay: square_avg starts at ONES and epsilon is added INSIDE
    the square root -- the two points where it differs from torch.optim.RMSprop"""

    def __init__(self, params, lr=7e-4, alpha=0.99, eps=1e-5):
        super().__init__(params, dict(lr=lr, alpha=alpha, eps=eps))

    @torch.no_grad()
    def step(self):
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                if not state:
                    state["square_avg"] = torch.ones_like(p)
                sq = state["square_avg"]
                sq.mul_(group["alpha"]).addcmul_(p.grad, p.grad, value=1 - group["alpha"])
                p.addcdiv_(p.grad, sq.add(group["eps"]).sqrt_(), value=-group["lr"])


def torch_update(model, opt, obs, act, adv, ret, vf_coef=1.0, ent=0.0, max_grad_norm=0.5, normalize_advantage=False):
    """A2C.train(): the minibatch body of train_ppo_torch.py::train with -(adv logp).mean() for the clipped surrogate, on all rows"""
    d = model.dist(obs)
    logp = d.log_prob(act).sum(-1)
    if normalize_advantage:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    pl = -(adv * logp).mean()
    vl = 0.5 * (model.v(obs).squeeze(-1) - ret / model.ret_scale).pow(2).mean()
    entropy = d.entropy().sum(-1).mean()
    loss = pl + vf_coef * vl - ent * entropy
    opt.zero_grad(set_to_none=True); loss.backward(); allreduce_mean_grads(model)
    torch.nn.utils.clip_grad_norm_(model.parameters(), max_grad_norm); opt.step()
    return pl.detach(), vl.detach(), entropy.detach()


def train(sim, model, iters, n_steps=5, lr=7e-4, alpha=0.99, rms_eps=1e-5, ent=0.0, vf_coef=1.0, gamma=0.99, lam=1.0, max_grad_norm=0.5,
          normalize_advantage=False, device_learner=False, seed=0, env_index_base=0, log=None, tag="", after_iter=None, log_every=100,
          vec_normalize=None):
    """`vec_normalize`: a DeviceVecNormalize that DeviceRollout puts between the simulator and its buffer.  `device_learner`: True builds a DeviceA2CLearner from `model`, an instance is used as it is.  -> (env steps taken, the learner
    or None).  `model` holds the current weights whenever after_iter runs and at the end"""
    from balance_robot_mujoco_rl_amd.learner import DeviceA2CLearner
    from balance_robot_mujoco_rl_amd.policy import DevicePolicy, DeviceRollout
    dev = sim.device
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    lrn = opt = None
    if device_learner:
        lrn = device_learner if isinstance(device_learner, DeviceA2CLearner) else DeviceA2CLearner(device=dev.index)
        lrn.lr, lrn.alpha, lrn.eps, lrn.vf_coef, lrn.ent_coef, lrn.max_grad_norm = lr, alpha, rms_eps, vf_coef, ent, max_grad_norm
        lrn.normalize_advantage = normalize_advantage
        lrn.load(model.state_dict())
    else:
        opt = RMSpropTFLike(model.parameters(), lr=lr, alpha=alpha, eps=rms_eps)
    pol = DevicePolicy(device=dev.index, seed=seed, env_index_base=env_index_base)
    mon = EpisodeMonitor(sim.n, device=dev.index)
    ro = DeviceRollout(sim, pol, n_steps, gamma=gamma, gae_lambda=lam, monitor=mon, normalize=vec_normalize)
    flat = lambda t: t.reshape((-1,) + t.shape[2:])
    seen, total, t_start = (0, 0.0, 0), 0, time.time()
    for it in range(iters):
        with torch.no_grad():
            pol.use_device_weights(flat_params(model) if lrn is None else lrn.rollout_params())
            ro.collect()
        obs, act, adv, ret = flat(ro.obs), flat(ro.action), flat(ro.adv), flat(ro.ret)
        if lrn is not None:   # one update over all n_steps x envs rows in buffer order (idx = None)
            _allreduce_mean_(lrn.grad(obs, act, adv, ret))
            lrn.apply()
        else:
            stats = torch_update(model, opt, obs, act, adv, ret, vf_coef, ent, max_grad_norm, normalize_advantage)
        total += sim.n * n_steps * world
        last = it == iters - 1
        if after_iter is not None or last or (log is not None and it % log_every == 0):
            if lrn is not None and (after_iter is not None or last):
                model.load_state_dict(lrn.state_dict())
            if log is not None and (it % log_every == 0 or last):
                st = mon.stats()
                d_len, d_ret, d_cnt = st.sum_len - seen[0], st.sum_ret - seen[1], st.episodes - seen[2]
                seen = (st.sum_len, st.sum_ret, st.episodes)
                if lrn is not None:
                    s = lrn.stats()
                    if s.bad_index:
                        raise RuntimeError(f"the device learner saw {s.bad_index} rows outside the rollout")
                    pl, vl, en = s.policy_loss, s.value_loss, s.entropy
                else:
                    pl, vl, en = (float(x) for x in stats)
                row = dict(tag=tag, iter=it, env_steps=total, wall_s=round(time.time() - t_start, 2), episodes=int(d_cnt),
                           mean_ep_len=d_len / d_cnt if d_cnt else None, mean_ep_ret=d_ret / d_cnt if d_cnt else None,
                           policy_loss=pl, value_loss=vl, entropy=en)
                log.append(row)
                if not dist.is_initialized() or dist.get_rank() == 0:
                    print(json.dumps(row), flush=True)
            if after_iter is not None:
                after_iter(it, model)
    torch.cuda.synchronize(dev)
    mon.close(); pol.close()
    return total, lrn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="Env01-v2"); ap.add_argument("--envs", type=int, default=16384, help="per rank")
    ap.add_argument("--iters", type=int, default=2000, help="rollouts = updates")
    ap.add_argument("--n-steps", type=int, default=5)
    ap.add_argument("--lr", type=float, default=7e-4); ap.add_argument("--alpha", type=float, default=0.99)
    ap.add_argument("--rms-eps", type=float, default=1e-5)
    ap.add_argument("--ent", type=float, default=0.0)
    ap.add_argument("--vf-coef", type=float, default=1.0,
                    help="on the value loss 0.5 (v - ret / ret_scale)^2: 1.0 here is SB3's vf_coef = 0.5 on mse_loss")
    ap.add_argument("--gamma", type=float, default=0.99); ap.add_argument("--lam", type=float, default=1.0)
    ap.add_argument("--max-grad-norm", type=float, default=0.5)
    ap.add_argument("--normalize-advantage", action="store_true")
    ap.add_argument("--log-std-init", type=float, default=0.0, help="SB3's default")
    ap.add_argument("--seed", type=int, default=0, help="seeds the initial weights, the action noise and the env streams")
    ap.add_argument("--eval-steps", type=int, default=0, help="after training: deterministic evaluation for this many steps")
    ap.add_argument("--eval-envs", type=int, default=4096)
    ap.add_argument("--eval-every", type=int, default=0, help="during training: evaluate_policy every this many iterations (rank 0)")
    ap.add_argument("--eval-episodes", type=int, default=1024)
    ap.add_argument("--save-best", default="")
    ap.add_argument("--device-learner", action="store_true", help="take the update with the HIP learner (brs_a2c_*) instead of torch")
    ap.add_argument("--vec-normalize", action="store_true",
                    help="SB3's VecNormalize on the device between the simulator and the rollout (one rank): running mean / variance "
                    "of the observations and of the discounted return, clipped at 10; the evaluations use the frozen statistics, "
                    "--save also writes them (<path>.vecnormalize.npz)")
    ap.add_argument("--save", default="", help="write the policy/value weights (torch state_dict) here")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if a.vec_normalize and world > 1:
        ap.error("--vec-normalize runs on one rank only: merging the running statistics across ranks is not implemented")
    rank = int(os.environ.get("RANK", "0")); local = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("BRS_PPO_ONE_DEVICE") == "1":
        local = 0
    if world > 1:
        torch.cuda.set_device(local)
        if os.environ.get("BRS_PPO_BACKEND", "nccl") == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(os.environ["BRS_PPO_BACKEND"])
    torch.manual_seed(a.seed)   # identical initial weights on every rank
    dev = torch.device("cuda", local)
    model = ActorCritic(a.log_std_init).to(dev)
    sim = BatchedSim(a.env, a.envs, device=local, seed=2 * a.seed, env_index_base=rank * a.envs, auto_reset=True)
    vecnorm = None
    if a.vec_normalize:
        from balance_robot_mujoco_rl_amd import DeviceVecNormalize
        vecnorm = DeviceVecNormalize(a.envs, device=local, gamma=a.gamma)
    cb = None
    if a.eval_every > 0 and rank == 0:
        cb = EvalCallback(a.env, a.eval_every, a.eval_episodes, min(a.eval_envs, a.eval_episodes), a.save_best, local, normalize=vecnorm)
    log = []
    t0 = time.perf_counter()
    total, _ = train(sim, model, a.iters, a.n_steps, a.lr, a.alpha, a.rms_eps, a.ent, a.vf_coef, a.gamma, a.lam, a.max_grad_norm,
                     a.normalize_advantage, a.device_learner, 1000 * (a.seed + 1), rank * a.envs, log, a.env, cb,
                     vec_normalize=vecnorm)
    wall = time.perf_counter() - t0
    sim.close()
    if world > 1:
        dist.barrier()
    if rank != 0:
        dist.destroy_process_group(); return
    run = dict(env_steps=total, wall_s=round(wall, 2), env_steps_per_s=round(total / wall))
    print(json.dumps(run), flush=True)
    evals = []
    if a.eval_steps > 0:
        evals.append(evaluate(a.env, model, a.eval_envs, a.eval_steps, normalize=vecnorm)); print(json.dumps(evals[-1]), flush=True)
    if a.save:
        torch.save(model.state_dict(), a.save)
        if vecnorm is not None:
            np.savez(a.save + ".vecnormalize.npz", **vecnorm.state_dict())
    if a.out:
        json.dump(dict(args=vars(a), world_size=world, run=run, log=log, eval=evals, eval_during_training=cb.rows if cb else []),
                  open(a.out, "w"), indent=1)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
