#!/usr/bin/env python3
"""Minimal DDPG on the batched simulator, SB3's defaults as arguments (the reference's second algorithm: src/sb_rl.py:72-83,
net_arch = dict(pi=[300, 200], qf=[200, 150]), NormalActionNoise(sigma=0.1)).  Two data paths:

  default         everything in torch: the buffer is a set of torch tensors, torch.randint samples it, the torch modules
                  compute the actions and the TD targets.  Runs on any device; the A/B baseline.
  --device-data   collection, buffer, sampling and TD targets by the HIP kernels (balance_robot_mujoco_rl_amd/offpolicy.py;
                  DESIGN.md 7.5).  The actor, the critic and the two targets are flat device tensors the kernels read in place; the
                  torch modules' parameters are VIEWS of them, so Adam's step and lerp_ on the flat vector (Polyak) are seen by the
                  next kernel without a copy.

In both paths torch does the critic loss mse(Q(s, a), y), the actor loss -mean Q(s, pi(s)), the two Adam steps and the Polyak
update, unless

  --device-learner  (with --device-data) the gradient step too is HIP kernels: DeviceDDPGLearner.step on the four flat vectors
                  (DESIGN.md 7.6).  The modules' parameters are views of them, so evaluation and state_dict keep working; the
                  logged losses are read once at the end.

Evaluation: evaluate_policy / EpisodeMonitor with sigma = 0."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ACTOR_SIZES, CRITIC_SIZES = (6, 300, 200, 2), (8, 200, 150, 1)


def mlp(sizes, squash):
    layers = []
    for k, (i, o) in enumerate(zip(sizes[:-1], sizes[1:])):
        layers.append(nn.Linear(i, o))
        if k < len(sizes) - 2:
            layers.append(nn.ReLU())
    return nn.Sequential(*layers, *([nn.Tanh()] if squash else []))


def flatten_module_(module, device):
    """move the module's parameters into ONE flat float32 tensor on `device`, in module order (weight, bias per Linear: the order
    of include/brs_policy.h), and make every parameter a view of it; -> the flat tensor"""
    ps = list(module.parameters())
    flat = torch.cat([p.detach().reshape(-1) for p in ps]).to(device=device, dtype=torch.float32).contiguous()
    at = 0
    for p in ps:
        k = p.numel()
        p.data = flat[at:at + k].view(p.shape)
        at += k
    return flat


class DDPG:
    """the four networks (state_dict keys actor.N / critic.N / actor_target.N / critic_target.N), their flat vectors, the two
    optimisers and the Polyak update"""

    def __init__(self, device, lr=1e-3, tau=0.005, seed=0):
        torch.manual_seed(seed)
        self.device, self.tau = torch.device(device), tau
        self.actor, self.critic = mlp(ACTOR_SIZES, True), mlp(CRITIC_SIZES, False)
        self.actor_target, self.critic_target = mlp(ACTOR_SIZES, True), mlp(CRITIC_SIZES, False)
        self.actor_target.load_state_dict(self.actor.state_dict()); self.critic_target.load_state_dict(self.critic.state_dict())
        self.flat = {k: flatten_module_(getattr(self, k), self.device) for k in ("actor", "critic", "actor_target", "critic_target")}
        for m in (self.actor_target, self.critic_target):
            m.requires_grad_(False)
        self.opt_actor = torch.optim.Adam(self.actor.parameters(), lr=lr)
        self.opt_critic = torch.optim.Adam(self.critic.parameters(), lr=lr)

    def state_dict(self):
        return {f"{net}.{k}": v for net in self.flat for k, v in getattr(self, net).state_dict().items()}

    def q(self, critic, obs, act):
        return critic(torch.cat([obs, act], dim=1)).squeeze(1)

    @torch.no_grad()
    def td_target_torch(self, next_obs, reward, done, gamma):
        return reward + (1.0 - done.float()) * gamma * self.q(self.critic_target, next_obs, self.actor_target(next_obs))

    def gradient_step(self, obs, action, y):
        """one critic step and one actor step on a minibatch with given targets, then the Polyak update; -> the two losses (tensors)"""
        critic_loss = nn.functional.mse_loss(self.q(self.critic, obs, action), y)
        self.opt_critic.zero_grad(set_to_none=True); critic_loss.backward(); self.opt_critic.step()
        actor_loss = -self.q(self.critic, obs, self.actor(obs)).mean()
        self.opt_actor.zero_grad(set_to_none=True); actor_loss.backward(); self.opt_actor.step()
        with torch.no_grad():
            self.flat["actor_target"].lerp_(self.flat["actor"], self.tau)
            self.flat["critic_target"].lerp_(self.flat["critic"], self.tau)
        return critic_loss.detach(), actor_loss.detach()


class TorchData:
    """the torch data path: act, buffer, sample, TD target; `sim` needs reset() and step() returning tensors on `device`"""

    def __init__(self, sim, model, cap, sigma, seed):
        self.sim, self.model, self.cap, self.sigma = sim, model, cap, sigma
        d, n = model.device, sim.n
        f = lambda *s: torch.zeros(s, dtype=torch.float32, device=d)
        self.obs, self.next_obs, self.action, self.reward = f(cap, n, 6), f(cap, n, 6), f(cap, n, 2), f(cap, n)
        self.done = torch.zeros((cap, n), dtype=torch.uint8, device=d)
        self.pos, self.full, self.last_obs = 0, False, None
        self.gen = torch.Generator(device=d); self.gen.manual_seed(seed)

    @torch.no_grad()
    def act(self, obs, random):
        n = obs.shape[0]
        mean = torch.rand((n, 2), generator=self.gen, device=obs.device) * 2 - 1 if random else self.model.actor(obs)
        return (mean + self.sigma * torch.randn((n, 2), generator=self.gen, device=obs.device)).clamp_(-1, 1)

    @torch.no_grad()
    def collect(self, steps, random, monitor=None):
        if self.last_obs is None:
            self.last_obs = self.sim.reset().clone()
        for _ in range(steps):
            a = self.act(self.last_obs, random)
            obs, rew, term, trunc, tobs = self.sim.step(a)
            if monitor is not None:
                monitor.update(rew, term, trunc)
            self.store(self.last_obs, a, obs, tobs, rew, term, trunc)
            self.last_obs.copy_(obs)

    @torch.no_grad()
    def store(self, last_obs, action, obs, terminal_obs, reward, terminated, truncated):
        p = self.pos
        ended = (terminated | truncated).bool()
        self.obs[p].copy_(last_obs); self.action[p].copy_(action); self.reward[p].copy_(reward)
        self.next_obs[p].copy_(torch.where(ended[:, None], terminal_obs, obs))
        self.done[p].copy_((terminated != 0).to(torch.uint8))   # a time-limit end bootstraps, a fall does not
        self.pos = (p + 1) % self.cap
        self.full = self.full or self.pos == 0

    @property
    def rows(self):
        return self.cap if self.full else self.pos

    @torch.no_grad()
    def sample(self, m):
        d = self.obs.device
        r = torch.randint(0, self.rows, (m,), generator=self.gen, device=d)
        e = torch.randint(0, self.sim.n, (m,), generator=self.gen, device=d)
        return self.obs[r, e], self.next_obs[r, e], self.action[r, e], self.reward[r, e], self.done[r, e]

    def td_target(self, next_obs, reward, done, gamma):
        return self.model.td_target_torch(next_obs, reward, done, gamma)


class DeviceData:
    """the --device-data path: the same four operations by the HIP kernels"""

    normalize = None   # a DeviceVecNormalize (--vec-normalize): the collector trains it, sample() normalises the minibatch with it

    def __init__(self, sim, model, cap, sigma, seed, monitor=None, normalize=None):
        from balance_robot_mujoco_rl_amd.offpolicy import DeviceDDPGNets, DeviceOffPolicyCollector, DeviceReplayBuffer
        self.sim, self.model, self.normalize = sim, model, normalize
        self.nets = DeviceDDPGNets(device=sim.device, seed=seed)
        self.replay = DeviceReplayBuffer(sim.n, cap, device=sim.device, seed=seed)
        self.collector = DeviceOffPolicyCollector(sim, self.nets, model.flat["actor"], self.replay, sigma=sigma, monitor=monitor,
                                                  normalize=normalize)
        self._y = None

    def collect(self, steps, random, monitor=None):
        self.collector.monitor = monitor
        self.collector.collect(steps, random=random)

    @property
    def rows(self):
        return self.replay.rows

    def sample(self, m):
        return self.replay.sample(m, normalize=self.normalize)

    def td_target(self, next_obs, reward, done, gamma):
        return self.nets.td_target(self.model.flat["actor_target"], self.model.flat["critic_target"], next_obs, reward, done, gamma)


def train(sim, model, data, steps, batch=256, learning_starts=100, gamma=0.99, gradient_steps=1, train_freq=1, monitor=None, log=None,
          learner=None):
    """`steps` env steps of every env: collect train_freq steps, then gradient_steps updates once learning_starts TRANSITIONS are
    in (SB3 counts num_timesteps over all envs); until then the actions are uniform.  `learner`: a DeviceDDPGLearner that takes
    the gradient step on model.flat instead of model.gradient_step"""
    losses, t, updates = [], 0, 0
    while t < steps:
        k = min(train_freq, steps - t)
        data.collect(k, random=t * sim.n < learning_starts, monitor=monitor)
        t += k
        if t * sim.n >= learning_starts and data.rows > 0:
            for _ in range(gradient_steps):
                obs, next_obs, action, reward, done = data.sample(batch)
                y = data.td_target(next_obs, reward, done, gamma)
                if learner is not None:
                    learner.step(model.flat, obs, action, y)
                else:
                    losses.append(model.gradient_step(obs, action, y))
                updates += 1
    if log is not None and losses:
        log["critic_loss_last"], log["actor_loss_last"] = (float(x) for x in losses[-1])
    if log is not None and learner is not None and updates:
        s = learner.stats()   # one read at the end, not one per update
        log["critic_loss_last"], log["actor_loss_last"] = s["critic_loss"], s["actor_loss"]
    return updates


def add_vec_normalize_argument(ap):
    ap.add_argument("--vec-normalize", action="store_true",
                    help="SB3's VecNormalize on the device (needs --device-data): the actor acts on normalised observations, the buffer "
                         "stores raw ones, every minibatch is normalised in the sampling kernel with the statistics of that moment; "
                         "evaluation runs on the frozen statistics; --save-actor P also writes P.vecnormalize.npz")


def check_vec_normalize(ap, a):
    """the two refusals of --vec-normalize, the PPO tool's"""
    if a.vec_normalize and not a.device_data:
        ap.error("--vec-normalize requires --device-data (it runs between the simulator and the HIP kernels of the data path)")
    if a.vec_normalize and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        ap.error("--vec-normalize runs on one rank only: merging the running statistics across ranks is not implemented")


def make_vec_normalize(a, sim):
    if not a.vec_normalize:
        return None
    from balance_robot_mujoco_rl_amd import DeviceVecNormalize
    return DeviceVecNormalize(a.envs, device=sim.device, gamma=a.gamma)


def save_vec_normalize(path, vecnorm):
    """next to the saved actor: the normaliser's state_dict (what vecnorm.fold_vecnormalize and eval_quant_policy.py --vec-normalize read)"""
    if vecnorm is not None:
        np.savez(path + ".vecnormalize.npz", **vecnorm.state_dict())


def normalized_act(act, normalize):
    """evaluation on frozen statistics: the stateless normalize_obs in front of `act`"""
    return act if normalize is None else (lambda obs, t: act(normalize.normalize_obs(obs), t))


def evaluate(env_id, model, episodes, envs, device_data, device=0, seed=123, normalize=None):
    """evaluate_policy with sigma = 0 -> (mean return, std, mean length); `normalize`: its statistics, frozen, in front of the actor"""
    from balance_robot_mujoco_rl_amd import BatchedSim, EpisodeMonitor, evaluate_policy
    sim = BatchedSim(env_id, envs, device=device, seed=seed, auto_reset=True)
    mon = EpisodeMonitor(envs, device=sim.device, max_len=max(1, int(sim.max_episode_steps)), log_capacity=episodes)
    if device_data:
        from balance_robot_mujoco_rl_amd.offpolicy import DeviceDDPGNets
        nets = DeviceDDPGNets(device=sim.device, seed=seed)
        act = normalized_act(lambda obs, t: nets.act(model.flat["actor"], obs, t, 0.0), normalize)
    else:
        def act(obs, t):
            with torch.no_grad():
                return model.actor(obs)
    ret, length = evaluate_policy(act, sim, n_eval_episodes=episodes, return_episode_rewards=True, monitor=mon)
    mon.close(); sim.close()
    return float(np.mean(ret)), float(np.std(ret)), float(np.mean(length))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="Env01-v1"); ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=1000, help="env steps of every env")
    ap.add_argument("--capacity-steps", type=int, default=0, help="rows of the buffer (default: SB3's 1,000,000 transitions / envs)")
    ap.add_argument("--lr", type=float, default=1e-3); ap.add_argument("--tau", type=float, default=0.005)
    ap.add_argument("--gamma", type=float, default=0.99); ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--learning-starts", type=int, default=100, help="transitions (over all envs) with uniform actions and no update")
    ap.add_argument("--sigma", type=float, default=0.1); ap.add_argument("--gradient-steps", type=int, default=1)
    ap.add_argument("--train-freq", type=int, default=1, help="env steps between two rounds of updates")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device-data", action="store_true", help="collection, buffer, sampling and TD targets by the HIP kernels")
    ap.add_argument("--device-learner", action="store_true", help="the gradient step by the HIP kernels too (needs --device-data)")
    ap.add_argument("--eval-episodes", type=int, default=0); ap.add_argument("--eval-envs", type=int, default=256)
    ap.add_argument("--out", default="")
    ap.add_argument("--save-actor", default="", help="write the trained actor on exit: the flat vector as .npy, or a state_dict as .pt "
                                                     "(either is what tools/eval_quant_policy.py --actor PATH --algo ddpg reads)")
    add_vec_normalize_argument(ap)
    a = ap.parse_args(argv)
    if a.device_learner and not a.device_data:
        ap.error("--device-learner requires --device-data")
    check_vec_normalize(ap, a)
    from balance_robot_mujoco_rl_amd import BatchedSim, EpisodeMonitor, _lib
    sim = BatchedSim(a.env, a.envs, device=0, seed=a.seed, auto_reset=True)
    cap = a.capacity_steps or max(1, 1_000_000 // a.envs)
    model = DDPG(sim.device, lr=a.lr, tau=a.tau, seed=a.seed)
    start = {k: v.clone() for k, v in model.flat.items()}
    monitor = EpisodeMonitor(a.envs, device=sim.device, max_len=max(1, int(sim.max_episode_steps)))
    vecnorm = make_vec_normalize(a, sim)
    data = DeviceData(sim, model, cap, a.sigma, a.seed, normalize=vecnorm) if a.device_data else TorchData(sim, model, cap, a.sigma, a.seed)
    log = {"args": vars(a), "build_id": _lib.build_id(), "data_path": "device" if a.device_data else "torch"}
    learner = None
    if a.device_learner:
        from balance_robot_mujoco_rl_amd.offpolicy import DeviceDDPGLearner
        learner = DeviceDDPGLearner(device=sim.device, max_batch=a.batch, lr=a.lr, tau=a.tau)
        log["learner"] = "device"
    torch.cuda.synchronize(); t0 = time.perf_counter()
    log["updates"] = train(sim, model, data, a.steps, a.batch, a.learning_starts, a.gamma, a.gradient_steps, a.train_freq, monitor, log,
                           learner=learner)
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
