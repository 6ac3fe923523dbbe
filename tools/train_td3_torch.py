#!/usr/bin/env python3
"""Minimal TD3 on the batched simulator: tools/train_ddpg_torch.py's recipe with TD3's three changes (SB3 TD3.train; the reference's
CLI offers `-a TD3` next to DDPG, src/sb_rl.py:73-83, :565) -- two critics and the minimum of their targets, clipped Gaussian noise on
the target action, and the actor and all targets updated only every `policy_delay`-th gradient step.  The widths stay the
reference's DDPG net_arch, pi=[300, 200], qf=[200, 150]: what policy_kwargs=dict(net_arch=dict(pi=[300, 200], qf=[200, 150])) gives
in SB3, not SB3's own TD3 default of [400, 300].  Three paths, as in the DDPG tool:

  default           everything in torch (the A/B baseline): buffer, sampling, target and `gradient_step`, written from SB3's rule.
  --device-data     collection, buffer, sampling and the TD3 target (DeviceDDPGNets.td3_target) by the HIP kernels; torch does the
                    two losses, the Adam steps and the Polyak updates on modules whose parameters are views of the flat vectors.
  --device-learner  (with --device-data) the update too is HIP kernels: DeviceTD3Learner.step.

The two critics are two modules (an nn.ModuleList: state_dict keys critic.0.N.* and critic.1.N.*) whose parameters are views of one
[2 NCRITIC] flat tensor, and likewise the targets.  Evaluation: evaluate_policy / EpisodeMonitor with sigma = 0."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from train_ddpg_torch import (ACTOR_SIZES, CRITIC_SIZES, DeviceData, TorchData, add_vec_normalize_argument, check_vec_normalize,  # noqa: E402
                              evaluate, flatten_module_, make_vec_normalize, mlp, save_vec_normalize)


class TD3:
    """the six networks (state_dict keys actor.N, critic.K.N, actor_target.N, critic_target.K.N), their four flat vectors (actor,
    critics, actor_target, critics_target), the two optimisers, the delay counter and the Polyak update"""

    def __init__(self, device, lr=1e-3, tau=0.005, seed=0, policy_delay=2, target_policy_noise=0.2, target_noise_clip=0.5):
        torch.manual_seed(seed)
        self.device, self.tau, self.policy_delay = torch.device(device), tau, int(policy_delay)
        self.policy_noise, self.noise_clip = float(target_policy_noise), float(target_noise_clip)
        twin = lambda: nn.ModuleList([mlp(CRITIC_SIZES, False), mlp(CRITIC_SIZES, False)])
        self.actor, self.critic, self.actor_target, self.critic_target = mlp(ACTOR_SIZES, True), twin(), mlp(ACTOR_SIZES, True), twin()
        self.actor_target.load_state_dict(self.actor.state_dict()); self.critic_target.load_state_dict(self.critic.state_dict())
        self.flat = {k: flatten_module_(getattr(self, m), self.device)
                     for k, m in (("actor", "actor"), ("critics", "critic"), ("actor_target", "actor_target"), ("critics_target", "critic_target"))}
        for m in (self.actor_target, self.critic_target):
            m.requires_grad_(False)
        self.opt_actor = torch.optim.Adam(self.actor.parameters(), lr=lr)
        self.opt_critics = torch.optim.Adam(self.critic.parameters(), lr=lr)   # one Adam over both critics
        self.gen = torch.Generator(device=self.device); self.gen.manual_seed(seed + 1)
        self.n_updates = 0

    def state_dict(self):
        return {f"{net}.{k}": v for net in ("actor", "critic", "actor_target", "critic_target") for k, v in getattr(self, net).state_dict().items()}

    def q(self, critic, obs, act):
        return critic(torch.cat([obs, act], dim=1)).squeeze(1)

    @torch.no_grad()
    def td_target_torch(self, next_obs, reward, done, gamma):
        """steps 1 to 4 of the rule: smoothing noise, its clip, the clamp of the action, the minimum of the two target critics"""
        z = torch.randn((next_obs.shape[0], 2), generator=self.gen, device=next_obs.device)
        eps = (self.policy_noise * z).clamp(-self.noise_clip, self.noise_clip)
        a = (self.actor_target(next_obs) + eps).clamp(-1.0, 1.0)
        q = torch.minimum(self.q(self.critic_target[0], next_obs, a), self.q(self.critic_target[1], next_obs, a))
        return reward + (1.0 - done.float()) * gamma * q

    def gradient_step(self, obs, action, y):
        """steps 5 and 6: the summed critic loss and one Adam step; every policy_delay-th update the actor's loss through the first,
        updated critic, its Adam step and the Polyak update of all targets; -> (critic loss, actor loss or None)"""
        self.n_updates += 1
        critic_loss = sum(nn.functional.mse_loss(self.q(c, obs, action), y) for c in self.critic)
        self.opt_critics.zero_grad(set_to_none=True); critic_loss.backward(); self.opt_critics.step()
        if self.n_updates % self.policy_delay != 0:
            return critic_loss.detach(), None
        actor_loss = -self.q(self.critic[0], obs, self.actor(obs)).mean()
        self.opt_actor.zero_grad(set_to_none=True); actor_loss.backward(); self.opt_actor.step()
        with torch.no_grad():
            self.flat["critics_target"].lerp_(self.flat["critics"], self.tau)
            self.flat["actor_target"].lerp_(self.flat["actor"], self.tau)
        return critic_loss.detach(), actor_loss.detach()


class TD3DeviceData(DeviceData):
    """the DDPG tool's device data path with the TD3 target: one brs_td3_td_target per minibatch, its draw counted here"""

    def __init__(self, sim, model, cap, sigma, seed, monitor=None, normalize=None):
        super().__init__(sim, model, cap, sigma, seed, monitor, normalize=normalize)
        self.target_draw = 0

    def td_target(self, next_obs, reward, done, gamma):
        m = self.model
        y = self.nets.td3_target(m.flat["actor_target"], m.flat["critics_target"], next_obs, reward, done, gamma, m.policy_noise, m.noise_clip,
                                 self.target_draw)
        self.target_draw += 1
        return y


def train(sim, model, data, steps, batch=256, learning_starts=100, gamma=0.99, gradient_steps=1, train_freq=1, monitor=None, log=None,
          learner=None):
    """the DDPG tool's loop: collect train_freq steps, then gradient_steps updates once learning_starts TRANSITIONS are in; until then
    the actions are uniform.  `learner`: a DeviceTD3Learner that takes the update on model.flat instead of model.gradient_step.
    -> (updates, actor updates)"""
    last_critic = last_actor = None
    t = updates = actor_updates = 0
    while t < steps:
        k = min(train_freq, steps - t)
        data.collect(k, random=t * sim.n < learning_starts, monitor=monitor)
        t += k
        if t * sim.n >= learning_starts and data.rows > 0:
            for _ in range(gradient_steps):
                obs, next_obs, action, reward, done = data.sample(batch)
                y = data.td_target(next_obs, reward, done, gamma)
                if learner is not None:
                    actor_updates += bool(learner.step(model.flat, obs, action, y))
                else:
                    last_critic, la = model.gradient_step(obs, action, y)
                    if la is not None:
                        last_actor, actor_updates = la, actor_updates + 1
                updates += 1
    if log is not None and learner is not None and updates:
        s = learner.stats()   # one read at the end, not one per update
        log["critic_loss_last"], log["mean_q1_last"], log["mean_q2_last"] = s["critic_loss"], s["mean_q1"], s["mean_q2"]
        if actor_updates:
            log["actor_loss_last"] = s["actor_loss"]
    elif log is not None and last_critic is not None:
        log["critic_loss_last"] = float(last_critic)
        if last_actor is not None:
            log["actor_loss_last"] = float(last_actor)
    return updates, actor_updates


def main(argv=None):
    ap = argparse.ArgumentParser(description="TD3 with the reference's DDPG net_arch on the batched simulator")
    ap.add_argument("--env", default="Env01-v1"); ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=1000, help="env steps of every env")
    ap.add_argument("--capacity-steps", type=int, default=0, help="rows of the buffer (default: SB3's 1,000,000 transitions / envs)")
    ap.add_argument("--lr", type=float, default=1e-3); ap.add_argument("--tau", type=float, default=0.005)
    ap.add_argument("--gamma", type=float, default=0.99); ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--learning-starts", type=int, default=100, help="transitions (over all envs) with uniform actions and no update")
    ap.add_argument("--policy-delay", type=int, default=2, help="the actor and all targets are updated every this many gradient steps")
    ap.add_argument("--target-policy-noise", type=float, default=0.2, help="standard deviation of the noise on the target action")
    ap.add_argument("--target-noise-clip", type=float, default=0.5, help="that noise is clipped to +- this")
    ap.add_argument("--sigma", type=float, default=0.1,
                    help="exploration noise on the collected actions.  SB3's TD3 has none by default and neither has the reference's generic "
                         "branch, so a deterministic actor would not explore at all: the DDPG recipe's NormalActionNoise(0.1) is kept")
    ap.add_argument("--gradient-steps", type=int, default=1)
    ap.add_argument("--train-freq", type=int, default=1, help="env steps between two rounds of updates")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device-data", action="store_true", help="collection, buffer, sampling and TD3 targets by the HIP kernels")
    ap.add_argument("--device-learner", action="store_true", help="the update by the HIP kernels too (needs --device-data)")
    ap.add_argument("--eval-episodes", type=int, default=0); ap.add_argument("--eval-envs", type=int, default=256)
    ap.add_argument("--out", default="")
    ap.add_argument("--save-actor", default="", help="write the trained actor on exit: the flat vector as .npy, or a state_dict as .pt "
                                                     "(either is what tools/eval_quant_policy.py --actor PATH --algo td3 reads)")
    add_vec_normalize_argument(ap)
    a = ap.parse_args(argv)
    if a.device_learner and not a.device_data:
        ap.error("--device-learner requires --device-data")
    check_vec_normalize(ap, a)
    if a.policy_delay < 1:
        ap.error("--policy-delay must be at least 1")
    if not (a.target_policy_noise >= 0 and a.target_noise_clip >= 0):
        ap.error("--target-policy-noise and --target-noise-clip must be >= 0")
    from balance_robot_mujoco_rl_amd import BatchedSim, EpisodeMonitor, _lib
    sim = BatchedSim(a.env, a.envs, device=0, seed=a.seed, auto_reset=True)
    cap = a.capacity_steps or max(1, 1_000_000 // a.envs)
    model = TD3(sim.device, lr=a.lr, tau=a.tau, seed=a.seed, policy_delay=a.policy_delay, target_policy_noise=a.target_policy_noise,
                target_noise_clip=a.target_noise_clip)
    start = {k: v.clone() for k, v in model.flat.items()}
    monitor = EpisodeMonitor(a.envs, device=sim.device, max_len=max(1, int(sim.max_episode_steps)))
    vecnorm = make_vec_normalize(a, sim)
    data = TD3DeviceData(sim, model, cap, a.sigma, a.seed, normalize=vecnorm) if a.device_data else TorchData(sim, model, cap, a.sigma, a.seed)
    log = {"args": vars(a), "build_id": _lib.build_id(), "data_path": "device" if a.device_data else "torch"}
    learner = None
    if a.device_learner:
        from balance_robot_mujoco_rl_amd.offpolicy import DeviceTD3Learner
        learner = DeviceTD3Learner(device=sim.device, max_batch=a.batch, lr=a.lr, tau=a.tau, policy_delay=a.policy_delay)
        log["learner"] = "device"
    torch.cuda.synchronize(); t0 = time.perf_counter()
    log["updates"], log["actor_updates"] = train(sim, model, data, a.steps, a.batch, a.learning_starts, a.gamma, a.gradient_steps, a.train_freq,
                                                 monitor, log, learner=learner)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    s = monitor.stats()
    log.update(seconds=dt, env_steps=a.steps * a.envs, env_steps_per_s=a.steps * a.envs / dt, monitor_steps=s.steps, train_episodes=s.episodes,
               train_mean_return=s.mean_ret, train_mean_len=s.mean_len,
               moved={k: float((model.flat[k] - start[k]).abs().max()) for k in start},
               finite=bool(all(torch.isfinite(v).all() for v in model.flat.values())))
    if a.eval_episodes:
        log["eval_mean_return"], log["eval_std_return"], log["eval_mean_len"] = evaluate(a.env, model, a.eval_episodes, a.eval_envs, a.device_data,
                                                                                         normalize=vecnorm)
    print(json.dumps(log))
    if a.save_actor:
        from balance_robot_mujoco_rl_amd import unflatten_ddpg_state_dict
        flat = model.flat["actor"].detach().cpu().numpy()
        if a.save_actor.endswith(".pt"):
            torch.save(unflatten_ddpg_state_dict(flat, "actor", "tool"), a.save_actor)
        else:
            np.save(a.save_actor, flat)
        save_vec_normalize(a.save_actor, vecnorm)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(log, f, indent=1)
    if learner is not None:
        learner.close()
    if vecnorm is not None:
        vecnorm.close()
    monitor.close(); sim.close()
    return log


if __name__ == "__main__":
    main()
