#!/usr/bin/env python3
"""Minimal SAC on the batched simulator: SB3's SAC.train and SACPolicy with SB3's defaults (ent_coef="auto" from 1.0,
target_entropy = -2, tau 0.005, gamma 0.99, lr 3e-4, batch 256, learning_starts 100, one update per step, no action noise, no gSDE;
the reference's CLI offers `-a SAC` next to DDPG and TD3, src/sb_rl.py:565) on the widths of tools/train_ddpg_torch.py and
tools/train_td3_torch.py, pi=[300, 200], qf=[200, 150], or with --net-arch sb3 on SB3's own [256, 256] for the actor and both
critics (what `sb_rl.py -a SAC` trains).  Three paths, as in the two siblings:

  default           everything in torch (the A/B baseline): buffer, sampling, target and `gradient_step`, written from SB3's rule.
  --device-data     collection (DeviceSACNets.act), buffer, sampling and the SAC target (DeviceSACNets.sac_target) by the HIP kernels;
                    torch does the losses, the Adam steps and the Polyak update on modules whose parameters are views of the flat
                    vectors.
  --device-learner  (with --device-data) the update too is HIP kernels: DeviceSACLearner.step.

The actor is three modules (state_dict keys actor.body.{0,2}.*, actor.mu.*, actor.log_std.*) whose parameters, with log_ent_coef
behind them, are views of one [SAC_NACTOR + 1] flat tensor in the kernels' order; the two critics are views of one [2 NCRITIC]
tensor as in the TD3 tool.  Evaluation: evaluate_policy / EpisodeMonitor with deterministic=True."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from train_ddpg_torch import (CRITIC_SIZES, DeviceData, TorchData, add_vec_normalize_argument, check_vec_normalize, flatten_module_,  # noqa: E402
                              make_vec_normalize, mlp, normalized_act, save_vec_normalize)

LOG_STD_MIN, LOG_STD_MAX, EPS = -20.0, 2.0, 1e-6
# --net-arch: the hidden widths of the actor and of the critics
NET_ARCHS = {"reference": ((300, 200), CRITIC_SIZES), "sb3": ((256, 256), (8, 256, 256, 1))}


class Actor(nn.Module):
    """SB3's SAC Actor: latent_pi (here `body`), then the two heads"""

    def __init__(self, hidden=(300, 200)):
        super().__init__()
        h1, h2 = hidden
        self.body = nn.Sequential(nn.Linear(6, h1), nn.ReLU(), nn.Linear(h1, h2), nn.ReLU())
        self.mu, self.log_std = nn.Linear(h2, 2), nn.Linear(h2, 2)

    def forward(self, obs):
        h = self.body(obs)
        return self.mu(h), torch.clamp(self.log_std(h), LOG_STD_MIN, LOG_STD_MAX)

    def action_log_prob(self, obs, z):
        """a = tanh(mu + std z) and its log-probability, as SB3's SquashedDiagGaussianDistribution writes it"""
        mu, log_std = self(obs)
        std = log_std.exp()
        u = mu + std * z
        logp = (-((u - mu) ** 2) / (2.0 * std ** 2) - log_std - 0.5 * math.log(2.0 * math.pi)).sum(dim=1)
        a = torch.tanh(u)
        return a, logp - torch.log(1.0 - a ** 2 + EPS).sum(dim=1)


class SAC:
    """the five networks (state_dict keys actor.body.N / actor.mu / actor.log_std, critic.K.N, critic_target.K.N, log_ent_coef), their
    three flat vectors (actor [SAC_NACTOR + 1] with log_ent_coef last, critics, critics_target), the optimisers and the Polyak update"""

    def __init__(self, device, lr=3e-4, tau=0.005, seed=0, ent_coef="auto", target_entropy=-2.0, net_arch="reference"):
        torch.manual_seed(seed)
        self.net_arch = net_arch
        pi_hidden, critic_sizes = NET_ARCHS[net_arch]
        self.device, self.tau, self.target_entropy = torch.device(device), tau, float(target_entropy)
        self.learn_alpha = ent_coef == "auto"
        twin = lambda: nn.ModuleList([mlp(critic_sizes, False), mlp(critic_sizes, False)])
        self.actor, self.critic, self.critic_target = Actor(pi_hidden), twin(), twin()
        self.critic_target.load_state_dict(self.critic.state_dict())
        self.log_ent_coef = nn.Parameter(torch.tensor([0.0 if self.learn_alpha else math.log(float(ent_coef))]), requires_grad=self.learn_alpha)
        a = self.actor
        ordered = [a.body[0].weight, a.body[0].bias, a.body[2].weight, a.body[2].bias, a.mu.weight, a.log_std.weight, a.mu.bias, a.log_std.bias,
                   self.log_ent_coef]   # W3[4][H2] = mu's rows, then log_std's; b3[4] likewise
        flat = torch.cat([p.detach().reshape(-1) for p in ordered]).to(device=self.device, dtype=torch.float32).contiguous()
        at = 0
        for p in ordered:
            p.data = flat[at:at + p.numel()].view(p.shape)
            at += p.numel()
        self.flat = {"actor": flat, "critics": flatten_module_(self.critic, self.device), "critics_target": flatten_module_(self.critic_target, self.device)}
        self.critic_target.requires_grad_(False)
        self.opt_actor = torch.optim.Adam(self.actor.parameters(), lr=lr)
        self.opt_ent = torch.optim.Adam([self.log_ent_coef], lr=lr) if self.learn_alpha else None
        self.opt_critics = torch.optim.Adam(self.critic.parameters(), lr=lr)   # one Adam over both critics
        self.gen = torch.Generator(device=self.device); self.gen.manual_seed(seed + 1)

    def state_dict(self):
        sd = {f"{net}.{k}": v for net in ("actor", "critic", "critic_target") for k, v in getattr(self, net).state_dict().items()}
        sd["log_ent_coef"] = self.log_ent_coef.detach()
        return sd

    def q(self, critic, obs, act):
        return critic(torch.cat([obs, act], dim=1)).squeeze(1)

    def min_q(self, critics, obs, act):
        return torch.min(torch.stack([self.q(c, obs, act) for c in critics], dim=1), dim=1)[0]

    def noise(self, n, z=None):
        return torch.randn((n, 2), generator=self.gen, device=self.device) if z is None else z

    @torch.no_grad()
    def td_target_torch(self, next_obs, reward, done, gamma, z=None):
        """the current actor on next_obs, the minimum of the two target critics, the entropy term"""
        a, logp = self.actor.action_log_prob(next_obs, self.noise(next_obs.shape[0], z))
        v = self.min_q(self.critic_target, next_obs, a) - torch.exp(self.log_ent_coef[0]) * logp
        return reward + (1.0 - done.float()) * gamma * v

    def gradient_step(self, obs, action, y, z=None):
        """SB3's order: the sample, the temperature's step (its value from BEFORE the step is used below), the critics' step on
        0.5 (mse1 + mse2), the actor's loss through the updated critics, the Polyak update; -> (critic loss, actor loss, ent_coef)"""
        a_pi, logp = self.actor.action_log_prob(obs, self.noise(obs.shape[0], z))
        ent_coef = torch.exp(self.log_ent_coef.detach())[0]
        if self.learn_alpha:
            ent_loss = -(self.log_ent_coef * (logp + self.target_entropy).detach()).mean()
            self.opt_ent.zero_grad(set_to_none=True); ent_loss.backward(); self.opt_ent.step()
        critic_loss = 0.5 * sum(nn.functional.mse_loss(self.q(c, obs, action), y) for c in self.critic)
        self.opt_critics.zero_grad(set_to_none=True); critic_loss.backward(); self.opt_critics.step()
        for c in self.critic:
            c.requires_grad_(False)
        actor_loss = (ent_coef * logp - self.min_q(self.critic, obs, a_pi)).mean()
        self.opt_actor.zero_grad(set_to_none=True); actor_loss.backward(); self.opt_actor.step()
        for c in self.critic:
            c.requires_grad_(True)
        with torch.no_grad():
            self.flat["critics_target"].lerp_(self.flat["critics"], self.tau)
        return critic_loss.detach(), actor_loss.detach(), ent_coef


class SACTorchData(TorchData):
    """the DDPG tool's torch data path with SAC's actor: no action noise, the policy's own sample"""

    @torch.no_grad()
    def act(self, obs, random):
        n = obs.shape[0]
        if random:
            return torch.rand((n, 2), generator=self.gen, device=obs.device) * 2 - 1
        return self.model.actor.action_log_prob(obs, torch.randn((n, 2), generator=self.gen, device=obs.device))[0]


class SACDeviceData(DeviceData):
    """the --device-data path: brs_sac_act in the collector, one brs_sac_td_target per minibatch, its draw counted here"""

    def __init__(self, sim, model, cap, seed, monitor=None, normalize=None):
        from balance_robot_mujoco_rl_amd.offpolicy import DeviceOffPolicyCollector, DeviceReplayBuffer, DeviceSACNets
        self.sim, self.model, self.normalize = sim, model, normalize
        self.nets = DeviceSACNets(device=sim.device, seed=seed, net_arch=model.net_arch)
        self.replay = DeviceReplayBuffer(sim.n, cap, device=sim.device, seed=seed)
        self.collector = DeviceOffPolicyCollector(sim, self.nets, model.flat["actor"], self.replay, sigma=0.0, monitor=monitor,
                                                  normalize=normalize)
        self.target_draw = 0

    def td_target(self, next_obs, reward, done, gamma):
        y = self.nets.sac_target(self.model.flat["actor"], self.model.flat["critics_target"], next_obs, reward, done, gamma, self.target_draw)
        self.target_draw += 1
        return y


def train(sim, model, data, steps, batch=256, learning_starts=100, gamma=0.99, gradient_steps=1, train_freq=1, monitor=None, log=None,
          learner=None):
    """the DDPG tool's loop: collect train_freq steps, then gradient_steps updates once learning_starts TRANSITIONS are in; until then
    the actions are uniform.  `learner`: a DeviceSACLearner that takes the update on model.flat instead of model.gradient_step.
    -> updates"""
    last = None
    t = updates = 0
    while t < steps:
        k = min(train_freq, steps - t)
        data.collect(k, random=t * sim.n < learning_starts, monitor=monitor)
        t += k
        if t * sim.n >= learning_starts and data.rows > 0:
            for _ in range(gradient_steps):
                obs, next_obs, action, reward, done = data.sample(batch)
                y = data.td_target(next_obs, reward, done, gamma)
                if learner is not None:
                    learner.step(model.flat, obs, action, y, updates)
                else:
                    last = model.gradient_step(obs, action, y)
                updates += 1
    if log is not None and learner is not None and updates:
        s = learner.stats()   # one read at the end, not one per update
        log["critic_loss_last"], log["actor_loss_last"], log["mean_logp_last"] = s["critic_loss"], s["actor_loss"], s["mean_logp"]
    elif log is not None and last is not None:
        log["critic_loss_last"], log["actor_loss_last"] = float(last[0]), float(last[1])
    if log is not None:
        log["ent_coef"] = float(torch.exp(model.flat["actor"][-1]))
    return updates


def evaluate(env_id, model, episodes, envs, device_data, device=0, seed=123, normalize=None):
    """evaluate_policy with deterministic=True -> (mean return, std, mean length); `normalize`: its statistics, frozen, in front of
    the actor"""
    from balance_robot_mujoco_rl_amd import BatchedSim, EpisodeMonitor, evaluate_policy
    sim = BatchedSim(env_id, envs, device=device, seed=seed, auto_reset=True)
    mon = EpisodeMonitor(envs, device=sim.device, max_len=max(1, int(sim.max_episode_steps)), log_capacity=episodes)
    if device_data:
        from balance_robot_mujoco_rl_amd.offpolicy import DeviceSACNets
        nets = DeviceSACNets(device=sim.device, seed=seed, net_arch=model.net_arch)
        act = normalized_act(lambda obs, t: nets.act(model.flat["actor"], obs, t, deterministic=True), normalize)
    else:
        def act(obs, t):
            with torch.no_grad():
                return torch.tanh(model.actor(obs)[0])
    ret, length = evaluate_policy(act, sim, n_eval_episodes=episodes, return_episode_rewards=True, monitor=mon)
    mon.close(); sim.close()
    return float(np.mean(ret)), float(np.std(ret)), float(np.mean(length))


def main(argv=None):
    ap = argparse.ArgumentParser(description="SAC with the reference's DDPG net_arch on the batched simulator")
    ap.add_argument("--env", default="Env01-v1"); ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=1000, help="env steps of every env")
    ap.add_argument("--capacity-steps", type=int, default=0, help="rows of the buffer (default: SB3's 1,000,000 transitions / envs)")
    ap.add_argument("--lr", type=float, default=3e-4); ap.add_argument("--tau", type=float, default=0.005)
    ap.add_argument("--gamma", type=float, default=0.99); ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--learning-starts", type=int, default=100, help="transitions (over all envs) with uniform actions and no update")
    ap.add_argument("--ent-coef", default="auto", help="'auto' (learned from 1.0, SB3's default) or a fixed positive number")
    ap.add_argument("--target-entropy", type=float, default=-2.0, help="SB3's 'auto' is -dim(action) = -2")
    ap.add_argument("--gradient-steps", type=int, default=1)
    ap.add_argument("--train-freq", type=int, default=1, help="env steps between two rounds of updates")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--net-arch", choices=sorted(NET_ARCHS), default="reference",
                    help="reference: pi=[300, 200], qf=[200, 150] (the reference's DDPG widths); sb3: SB3's default [256, 256]")
    ap.add_argument("--device-data", action="store_true", help="collection, buffer, sampling and SAC targets by the HIP kernels")
    ap.add_argument("--device-learner", action="store_true", help="the update by the HIP kernels too (needs --device-data)")
    ap.add_argument("--eval-episodes", type=int, default=0); ap.add_argument("--eval-envs", type=int, default=256)
    ap.add_argument("--out", default="")
    ap.add_argument("--save-actor", default="", help="write the trained actor on exit: the flat vector as .npy, or a state_dict as .pt "
                                                     "(either is what tools/eval_quant_policy.py --actor PATH --algo sac reads)")
    add_vec_normalize_argument(ap)
    a = ap.parse_args(argv)
    if a.device_learner and not a.device_data:
        ap.error("--device-learner requires --device-data")
    check_vec_normalize(ap, a)
    if a.ent_coef != "auto":
        try:
            ok = float(a.ent_coef) > 0 and math.isfinite(float(a.ent_coef))
        except ValueError:
            ok = False
        if not ok:
            ap.error("--ent-coef must be 'auto' or a positive number")
    if not math.isfinite(a.target_entropy):
        ap.error("--target-entropy must be finite")
    from balance_robot_mujoco_rl_amd import BatchedSim, EpisodeMonitor, _lib
    sim = BatchedSim(a.env, a.envs, device=0, seed=a.seed, auto_reset=True)
    cap = a.capacity_steps or max(1, 1_000_000 // a.envs)
    model = SAC(sim.device, lr=a.lr, tau=a.tau, seed=a.seed, ent_coef=a.ent_coef, target_entropy=a.target_entropy, net_arch=a.net_arch)
    start = {k: v.clone() for k, v in model.flat.items()}
    monitor = EpisodeMonitor(a.envs, device=sim.device, max_len=max(1, int(sim.max_episode_steps)))
    vecnorm = make_vec_normalize(a, sim)
    data = SACDeviceData(sim, model, cap, a.seed, normalize=vecnorm) if a.device_data else SACTorchData(sim, model, cap, 0.0, a.seed)
    log = {"args": vars(a), "build_id": _lib.build_id(), "data_path": "device" if a.device_data else "torch"}
    learner = None
    if a.device_learner:
        from balance_robot_mujoco_rl_amd.offpolicy import DeviceSACLearner
        learner = DeviceSACLearner(device=sim.device, max_batch=a.batch, lr=a.lr, tau=a.tau, target_entropy=a.target_entropy,
                                   learn_alpha=model.learn_alpha, seed=a.seed, net_arch=a.net_arch)
        log["learner"] = "device"
    torch.cuda.synchronize(); t0 = time.perf_counter()
    log["updates"] = train(sim, model, data, a.steps, a.batch, a.learning_starts, a.gamma, a.gradient_steps, a.train_freq, monitor, log, learner=learner)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    s = monitor.stats()
    log.update(seconds=dt, env_steps=a.steps * a.envs, env_steps_per_s=a.steps * a.envs / dt, monitor_steps=s.steps, train_episodes=s.episodes,
               train_mean_return=s.mean_ret, train_mean_len=s.mean_len,
               moved={**{k: float((model.flat[k] - start[k]).abs().max()) for k in start},
                      "log_ent_coef": float((model.flat["actor"][-1] - start["actor"][-1]).abs())},
               finite=bool(all(torch.isfinite(v).all() for v in model.flat.values())))
    if a.eval_episodes:
        log["eval_mean_return"], log["eval_std_return"], log["eval_mean_len"] = evaluate(a.env, model, a.eval_episodes, a.eval_envs, a.device_data,
                                                                                         normalize=vecnorm)
    print(json.dumps(log))
    if a.save_actor:
        from balance_robot_mujoco_rl_amd import unflatten_sac_actor
        flat = model.flat["actor"].detach().cpu().numpy()
        if a.save_actor.endswith(".pt"):
            torch.save(unflatten_sac_actor(flat, "tool"), a.save_actor)
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
