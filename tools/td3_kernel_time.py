#!/usr/bin/env python3
"""What TD3 costs on the device, the measurements that end up in profiles/td3_kernel_stats.json (each mode adds its
section to --out), the profiler off.  The method is tools/ddpg_learner_kernel_time.py's: a warm-up of 10, three repeats of --calls,
the sides alternating in the same process, medians and all repeats written down, the build id in the file, m = 256 and m = 8,192.

  --kernels  (a) brs_td3_td_target against torch's target of tools/train_td3_torch.py, next to brs_ddpg_td_target;
             (b) brs_ddpg_learner_twin_critic_grad against two consecutive brs_ddpg_learner_critic_grad calls;
             (c) the whole update against torch's gradient_step, delayed and non-delayed steps separately
  --wall     (d) DESIGN.md 7.5's run with the TD3 tool: Env01-v1, --envs envs, --steps env steps, one update of batch 256 per step,
             torch, then --device-data, then --device-data --device-learner, after a 20-step warm-up run
  --train    (e) one run as found: --train-envs envs x --train-steps steps on the device path, then 64 evaluation episodes, sigma = 0
      python3 tools/td3_kernel_time.py --kernels --wall --train --out profiles/td3_kernel_stats.json
"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ddpg_learner_kernel_time import _alternate, _emit  # noqa: E402
SIGMA, GAMMA, NOISE, CLIP = 0.1, 0.99, 0.2, 0.5


def _sides(t):
    out = {k + "_us": [round(x, 2) for x in v] for k, v in t.items()}
    out.update({k + "_median_us": round(statistics.median(v), 2) for k, v in t.items()})
    return out


def kernels(calls):
    import torch
    import train_td3_torch as T
    from balance_robot_mujoco_rl_amd import DeviceDDPGLearner, DeviceDDPGNets, DeviceTD3Learner
    from balance_robot_mujoco_rl_amd.offpolicy import NCRITIC
    dev = torch.device("cuda", 0)
    res = {"calls_per_repeat": calls, "repeats": 3, "warmup": 10, "units": "microseconds per call", "sizes": {}}
    nets = DeviceDDPGNets(device=0, seed=0)
    for m in (256, 8192):
        gen = torch.Generator(device=dev); gen.manual_seed(m)
        scale = torch.tensor([1.5, 4.0, 0.5, 0.5, 0.5, 0.5], device=dev)
        obs, next_obs = (torch.randn((m, 6), generator=gen, device=dev) * scale for _ in range(2))
        act = torch.rand((m, 2), generator=gen, device=dev) * 2 - 1
        y, reward = torch.randn(m, generator=gen, device=dev), torch.randn(m, generator=gen, device=dev)
        done = (torch.arange(m, device=dev) % 3 == 1).to(torch.uint8)
        t_model, d_model = T.TD3(dev, seed=0), T.TD3(dev, seed=0)   # the same initial weights, one set per side
        f = d_model.flat
        twin, single = DeviceTD3Learner(device=0, max_batch=m, policy_delay=2), DeviceDDPGLearner(device=0, max_batch=m)
        y_out, draw = torch.empty(m, device=dev), [0]

        def td3_target():
            nets.td3_target(f["actor_target"], f["critics_target"], next_obs, reward, done, GAMMA, NOISE, CLIP, draw[0], out=y_out)
            draw[0] += 1
        c0, c1, g1 = f["critics"][:NCRITIC], f["critics"][NCRITIC:], torch.zeros_like(single.grad_critic)

        def two_single():
            single.critic_grad(c0, obs, act, y)
            single.critic_grad(c1, obs, act, y, out=g1)
        a = _alternate(torch, {"torch_target": lambda: t_model.td_target_torch(next_obs, reward, done, GAMMA), "td3_target": td3_target,
                               "ddpg_target": lambda: nets.td_target(f["actor_target"], f["critics_target"][:NCRITIC], next_obs, reward, done, GAMMA,
                                                                     out=y_out)}, calls)
        b = _alternate(torch, {"twin_critic_grad": lambda: twin.twin_critic_grad(f["critics"], obs, act, y), "two_critic_grad_calls": two_single,
                               "one_critic_grad_call": lambda: single.critic_grad(c0, obs, act, y)}, calls)

        def torch_step(delayed):
            def run():
                t_model.n_updates = 1 if delayed else 0   # gradient_step counts first: 2 is a delayed update, 1 is not
                t_model.gradient_step(obs, act, y)
            return run

        def device_step(delayed):
            def run():
                twin.n_updates = 1 if delayed else 0
                twin.step(f, obs, act, y)
            return run
        c = _alternate(torch, {"torch_delayed": torch_step(True), "device_delayed": device_step(True), "torch_not_delayed": torch_step(False),
                               "device_not_delayed": device_step(False)}, calls)
        ma, mb, mc = ({k: statistics.median(v) for k, v in t.items()} for t in (a, b, c))
        res["sizes"][f"m{m}"] = dict(
            target=dict(**_sides(a), torch_over_td3=round(ma["torch_target"] / ma["td3_target"], 2), td3_minus_ddpg_us=round(ma["td3_target"] - ma["ddpg_target"], 2)),
            critic_grad=dict(**_sides(b), two_calls_over_twin=round(mb["two_critic_grad_calls"] / mb["twin_critic_grad"], 2)),
            update=dict(**_sides(c), torch_over_device_delayed=round(mc["torch_delayed"] / mc["device_delayed"], 2),
                        torch_over_device_not_delayed=round(mc["torch_not_delayed"] / mc["device_not_delayed"], 2)),
            finite=bool(all(torch.isfinite(v).all() for v in list(f.values()) + list(t_model.flat.values()))))
        twin.close(); single.close()
    nets.close()
    return res


def _run(mode, envs, steps, seed=0, eval_episodes=0):
    import torch
    import train_td3_torch as T
    from balance_robot_mujoco_rl_amd import BatchedSim, DeviceTD3Learner, EpisodeMonitor
    sim = BatchedSim("Env01-v1", envs, device=0, seed=seed, auto_reset=True)
    model = T.TD3(sim.device, seed=seed, target_policy_noise=NOISE, target_noise_clip=CLIP)
    mon = EpisodeMonitor(envs, device=0, max_len=int(sim.max_episode_steps))
    cap = max(1, 1_000_000 // envs)
    data = T.TorchData(sim, model, cap, SIGMA, seed) if mode == "torch" else T.TD3DeviceData(sim, model, cap, SIGMA, seed)
    learner = DeviceTD3Learner(device=0, max_batch=256, policy_delay=2) if mode == "device_data_device_learner" else None
    log = {}
    torch.cuda.synchronize(); t0 = time.perf_counter()
    updates, actor_updates = T.train(sim, model, data, steps, batch=256, learning_starts=100, gamma=GAMMA, gradient_steps=1, train_freq=1, monitor=mon,
                                     log=log, learner=learner)
    torch.cuda.synchronize(); wall = time.perf_counter() - t0
    s = mon.stats()
    out = dict(mode=mode, envs=envs, steps=steps, updates=updates, actor_updates=actor_updates, wall_s=round(wall, 3),
               env_steps_per_s=round(steps * envs / wall), train_episodes=s.episodes, train_mean_len=s.mean_len, **log,
               finite=bool(all(torch.isfinite(v).all() for v in model.flat.values())))
    if eval_episodes:
        out["eval_episodes"] = eval_episodes
        out["eval_mean_return"], out["eval_std_return"], out["eval_mean_len"] = T.evaluate("Env01-v1", model, eval_episodes, 64, mode != "torch")
    if learner is not None:
        learner.close()
    mon.close(); sim.close()
    return out


def wall(envs, steps):
    res = {"recipe": f"Env01-v1, {envs} envs, {steps} env steps, one TD3 update of batch 256 per env step (policy_delay 2, target noise 0.2 / 0.5, "
                     "sigma 0.1), SB3's defaults otherwise", "runs": []}
    _run("device_data_device_learner", envs, 20)   # warm-up: library load, first launches, allocator
    for mode in ("torch", "device_data", "device_data_device_learner"):
        res["runs"].append(_run(mode, envs, steps))
    base = res["runs"][0]["env_steps_per_s"]
    res["over_torch_env_steps_per_s"] = {r["mode"]: round(r["env_steps_per_s"] / base, 2) for r in res["runs"][1:]}
    return res


def train(envs, steps):
    return {"recipe": f"Env01-v1, {envs} envs x {steps} env steps on the device path, nothing tuned, then 64 evaluation episodes with sigma = 0 "
                      "(an episode lasts at most 6,000 steps)", "run": _run("device_data_device_learner", envs, steps, eval_episodes=64)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true"); ap.add_argument("--wall", action="store_true"); ap.add_argument("--train", action="store_true")
    ap.add_argument("--calls", type=int, default=200); ap.add_argument("--envs", type=int, default=16384); ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--train-envs", type=int, default=256); ap.add_argument("--train-steps", type=int, default=2000)
    ap.add_argument("--out", default="", help="JSON file to add this mode's section to")
    a = ap.parse_args()
    if a.kernels:
        _emit("kernels", kernels(a.calls), a.out)
    if a.wall:
        _emit("wall", wall(a.envs, a.steps), a.out)
    if a.train:
        _emit("train", train(a.train_envs, a.train_steps), a.out)


if __name__ == "__main__":
    main()
