#!/usr/bin/env python3
"""What the DDPG gradient step costs, two measurements that end up in profiles/ddpg_learner_kernel_stats.json
(each mode adds its section to --out), the profiler off:

  step time  microseconds per full gradient step (critic gradient, Adam, actor gradient through the updated critic, Adam, both
             Polyak updates) at m = 256 and m = 8,192: DDPG.gradient_step of tools/train_ddpg_torch.py and DeviceDDPGLearner.step
             on the same tensors, alternating, medians of three repeats of --calls steps after a warm-up; and the device step
             call by call (each of the four calls alone, same method)
      python3 tools/ddpg_learner_kernel_time.py --step-time --out profiles/ddpg_learner_kernel_stats.json
  wall       DESIGN.md 7.5's run again: Env01-v1, --envs envs, --steps env steps, one update of batch 256 per step, three ways:
             torch, --device-data, --device-data --device-learner: env-steps/s of each
      python3 tools/ddpg_learner_kernel_time.py --wall --out profiles/ddpg_learner_kernel_stats.json
"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
SIGMA, GAMMA = 0.1, 0.99


def _alternate(torch, sides, calls, warmup=10):
    """sides: {name: f()} -> {name: [us per call] x 3}, alternating so that all see the same clocks"""
    for f in sides.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in sides}
    for _ in range(3):
        for name, f in sides.items():
            t0 = time.perf_counter()
            for _ in range(calls):
                f()
            torch.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) / calls * 1e6)
    return t


def step_time(calls):
    import torch
    import train_ddpg_torch as T
    from balance_robot_mujoco_rl_amd import DeviceDDPGLearner
    dev = torch.device("cuda", 0)
    res = {"calls_per_repeat": calls, "repeats": 3, "units": "microseconds per gradient step", "sizes": {}}
    for m in (256, 8192):
        gen = torch.Generator(device=dev); gen.manual_seed(m)
        obs = torch.randn((m, 6), generator=gen, device=dev) * torch.tensor([1.5, 4.0, 0.5, 0.5, 0.5, 0.5], device=dev)
        act = torch.rand((m, 2), generator=gen, device=dev) * 2 - 1
        y = torch.randn(m, generator=gen, device=dev)
        t_model, d_model = T.DDPG(dev, seed=0), T.DDPG(dev, seed=0)   # the same initial weights, one set per side
        lrn = DeviceDDPGLearner(device=0, max_batch=m)
        f = d_model.flat
        t = _alternate(torch, {"torch": lambda: t_model.gradient_step(obs, act, y), "device": lambda: lrn.step(f, obs, act, y)}, calls)
        med = {k: statistics.median(v) for k, v in t.items()}
        parts = _alternate(torch, {"critic_grad": lambda: lrn.critic_grad(f["critic"], obs, act, y),
                                   "apply_critic": lambda: lrn.apply_critic(f["critic"], f["critic_target"]),
                                   "actor_grad": lambda: lrn.actor_grad(f["actor"], f["critic"], obs),
                                   "apply_actor": lambda: lrn.apply_actor(f["actor"], f["actor_target"])}, calls)
        res["sizes"][f"m{m}"] = dict(torch_us=[round(x, 2) for x in t["torch"]], device_us=[round(x, 2) for x in t["device"]],
                                     torch_median_us=round(med["torch"], 2), device_median_us=round(med["device"], 2),
                                     torch_over_device=round(med["torch"] / med["device"], 2),
                                     device_calls_median_us={k: round(statistics.median(v), 2) for k, v in parts.items()},
                                     finite=bool(all(torch.isfinite(v).all() for v in list(f.values()) + list(t_model.flat.values()))))
        lrn.close()
    return res


def _run(mode, envs, steps, seed=0):
    import torch
    import train_ddpg_torch as T
    from balance_robot_mujoco_rl_amd import BatchedSim, DeviceDDPGLearner, EpisodeMonitor
    sim = BatchedSim("Env01-v1", envs, device=0, seed=seed, auto_reset=True)
    model = T.DDPG(sim.device, seed=seed)
    mon = EpisodeMonitor(envs, device=0, max_len=int(sim.max_episode_steps))
    cap = max(1, 1_000_000 // envs)
    data = T.TorchData(sim, model, cap, SIGMA, seed) if mode == "torch" else T.DeviceData(sim, model, cap, SIGMA, seed)
    learner = DeviceDDPGLearner(device=0, max_batch=256) if mode == "device_data_device_learner" else None
    log = {}
    torch.cuda.synchronize(); t0 = time.perf_counter()
    updates = T.train(sim, model, data, steps, batch=256, learning_starts=100, gamma=GAMMA, gradient_steps=1, train_freq=1, monitor=mon, log=log,
                      learner=learner)
    torch.cuda.synchronize(); wall = time.perf_counter() - t0
    out = dict(mode=mode, envs=envs, steps=steps, updates=updates, wall_s=round(wall, 3), env_steps_per_s=round(steps * envs / wall), **log,
               finite=bool(all(torch.isfinite(v).all() for v in model.flat.values())))
    if learner is not None:
        learner.close()
    mon.close(); sim.close()
    return out


def wall(envs, steps):
    res = {"recipe": f"Env01-v1, {envs} envs, {steps} env steps, one update of batch 256 per env step, SB3's defaults otherwise", "runs": []}
    _run("device_data_device_learner", envs, 20)   # warm-up: library load, first launches, allocator
    for mode in ("torch", "device_data", "device_data_device_learner"):
        res["runs"].append(_run(mode, envs, steps))
    base = res["runs"][0]["env_steps_per_s"]
    res["over_torch_env_steps_per_s"] = {r["mode"]: round(r["env_steps_per_s"] / base, 2) for r in res["runs"][1:]}
    return res


def _emit(section, res, out):
    from balance_robot_mujoco_rl_amd import _lib
    if out:
        doc = json.load(open(out)) if os.path.exists(out) else {}
        doc["build_id"] = _lib.build_id()
        doc[section] = res
        json.dump(doc, open(out, "w"), indent=1)
    print(json.dumps({section: res}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step-time", action="store_true"); ap.add_argument("--wall", action="store_true")
    ap.add_argument("--calls", type=int, default=200); ap.add_argument("--envs", type=int, default=16384); ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default="", help="JSON file to add this mode's section to")
    a = ap.parse_args()
    if a.step_time:
        _emit("step_time", step_time(a.calls), a.out)
    if a.wall:
        _emit("wall", wall(a.envs, a.steps), a.out)


if __name__ == "__main__":
    main()
