#!/usr/bin/env python3
"""What the DDPG data path costs, three measurements that end up in profiles/offpolicy_kernel_stats.json (each
mode adds its section to --out):

  op time    profiler off: microseconds per call of the five device operations and of the torch path of tools/train_ddpg_torch.py
             doing the same work on the same tensors -- act and q at n = 65,536, add at n = 65,536, td_target and sample at
             m = 256 and 8,192 from a 16-row buffer of 65,536 envs -- the two alternating, three repeats each, median over the
             repeats of the mean of --calls calls after a warm-up; and the Env03-v2 env step at 65,536 envs in the same run
      python3 tools/offpolicy_kernel_time.py --op-time --out profiles/offpolicy_kernel_stats.json
  wall       one fixed short run of the tool (same seeds) with --device-data off and on: env-steps/s of both
      python3 tools/offpolicy_kernel_time.py --wall --out profiles/offpolicy_kernel_stats.json
  balance    does the recipe balance Env01-v1 with SB3's defaults?  One longer --device-data run and its evaluation, as found
      python3 tools/offpolicy_kernel_time.py --balance --out profiles/offpolicy_kernel_stats.json
"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
N, CAP, SIGMA, GAMMA = 65536, 16, 0.1, 0.99


class _Envs:
    """what TorchData needs of a simulator when it is only asked to store and sample"""

    def __init__(self, n):
        self.n = n


def _alternate(torch, sides, calls):
    """sides: {name: f(k)} -> {name: [us per call] x 3}, alternating so that both see the same clocks"""
    for f in sides.values():
        for k in range(10):
            f(k)
    torch.cuda.synchronize()
    t = {k: [] for k in sides}
    for _ in range(3):
        for name, f in sides.items():
            t0 = time.perf_counter()
            for k in range(calls):
                f(k)
            torch.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) / calls * 1e6)
    return t


def _row(t):
    med = {k: statistics.median(v) for k, v in t.items()}
    return dict(torch_us=[round(x, 2) for x in t["torch"]], device_us=[round(x, 2) for x in t["device"]], torch_median_us=round(med["torch"], 2),
                device_median_us=round(med["device"], 2), torch_over_device=round(med["torch"] / med["device"], 2))


def op_time(calls):
    import torch
    import train_ddpg_torch as T
    from balance_robot_mujoco_rl_amd import BatchedSim, DeviceDDPGNets, DeviceReplayBuffer
    dev = torch.device("cuda", 0)
    model = T.DDPG(dev, seed=0)
    nets = DeviceDDPGNets(device=0, seed=0)
    sim = BatchedSim("Env03-v2", N, device=0, seed=0, auto_reset=True)
    obs = sim.reset().clone()
    res = {"n": N, "buffer_rows": CAP, "calls_per_repeat": calls, "repeats": 3, "units": "microseconds per call", "ops": {}}
    # the env step the actor feeds, in the same run
    act = torch.zeros((N, 2), device=dev)
    for _ in range(10):
        sim.step(act)
    torch.cuda.synchronize()
    steps = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(calls):
            out = sim.step(act)
        torch.cuda.synchronize()
        steps.append((time.perf_counter() - t0) / calls * 1e6)
    res["env_step_us"] = [round(x, 2) for x in steps]
    new_obs, rew, term, trunc, tobs = (x.clone() for x in out)
    td = T.TorchData(_Envs(N), model, CAP, SIGMA, 0)
    replay = DeviceReplayBuffer(N, CAP, device=0, seed=0)
    a_dev, q_dev = torch.empty((N, 2), device=dev), torch.empty(N, device=dev)
    with torch.no_grad():
        res["ops"]["act_n65536"] = _row(_alternate(torch, {"torch": lambda k: td.act(obs, False),
                                                           "device": lambda k: nets.act(model.flat["actor"], obs, k, SIGMA, out=a_dev)}, calls))
        res["ops"]["act_n65536"]["device_share_of_env_step"] = round(res["ops"]["act_n65536"]["device_median_us"] / statistics.median(steps), 4)
        res["ops"]["act_n65536"]["torch_share_of_env_step"] = round(res["ops"]["act_n65536"]["torch_median_us"] / statistics.median(steps), 4)
        res["ops"]["q_n65536"] = _row(_alternate(torch, {"torch": lambda k: model.q(model.critic, obs, a_dev),
                                                         "device": lambda k: nets.q(model.flat["critic"], obs, a_dev, out=q_dev)}, calls))
        res["ops"]["add_n65536"] = _row(_alternate(torch, {"torch": lambda k: td.store(obs, a_dev, new_obs, tobs, rew, term, trunc),
                                                           "device": lambda k: replay.add(obs, a_dev, new_obs, tobs, rew, term, trunc)}, calls))
        for m in (256, 8192):
            batch = replay.new_batch(m)
            y = torch.empty(m, device=dev)
            res["ops"][f"sample_m{m}"] = _row(_alternate(torch, {"torch": lambda k: td.sample(m), "device": lambda k: replay.sample(m, out=batch)}, calls))
            o, no, a, r, d = batch
            res["ops"][f"td_target_m{m}"] = _row(_alternate(torch, {
                "torch": lambda k: model.td_target_torch(no, r, d, GAMMA),
                "device": lambda k: nets.td_target(model.flat["actor_target"], model.flat["critic_target"], no, r, d, GAMMA, out=y)}, calls))
    sim.close(); nets.close()
    return res


def _run(device_data, env, envs, steps, gradient_steps, seed=0, eval_episodes=0):
    import torch
    import train_ddpg_torch as T
    from balance_robot_mujoco_rl_amd import BatchedSim, EpisodeMonitor
    sim = BatchedSim(env, envs, device=0, seed=seed, auto_reset=True)
    model = T.DDPG(sim.device, seed=seed)
    mon = EpisodeMonitor(envs, device=0, max_len=int(sim.max_episode_steps))
    cap = max(1, 1_000_000 // envs)
    data = T.DeviceData(sim, model, cap, SIGMA, seed) if device_data else T.TorchData(sim, model, cap, SIGMA, seed)
    log = {}
    torch.cuda.synchronize(); t0 = time.perf_counter()
    updates = T.train(sim, model, data, steps, batch=256, learning_starts=100, gamma=GAMMA, gradient_steps=gradient_steps, train_freq=1, monitor=mon, log=log)
    torch.cuda.synchronize(); wall = time.perf_counter() - t0
    s = mon.stats()
    out = dict(device_data=device_data, env=env, envs=envs, steps=steps, updates=updates, wall_s=round(wall, 3), env_steps_per_s=round(steps * envs / wall),
               train_episodes=s.episodes, train_mean_return=s.mean_ret, train_mean_len=s.mean_len, **log,
               finite=bool(all(torch.isfinite(v).all() for v in model.flat.values())))
    mon.close(); sim.close()
    if eval_episodes:
        mean, std, length = T.evaluate(env, model, eval_episodes, min(eval_episodes, 256), device_data)
        out.update(eval_episodes=eval_episodes, eval_mean_return=round(mean, 3), eval_std_return=round(std, 3), eval_mean_len=round(length, 2))
    return out


def wall(envs, steps):
    res = {"recipe": f"Env01-v1, {envs} envs, {steps} env steps, one update of batch 256 per env step, SB3's defaults otherwise", "runs": []}
    _run(True, "Env01-v1", envs, 20, 1)   # warm-up: library load, first launches, allocator
    for device_data in (False, True):
        res["runs"].append(_run(device_data, "Env01-v1", envs, steps, 1))
    res["device_over_torch_env_steps_per_s"] = round(res["runs"][1]["env_steps_per_s"] / res["runs"][0]["env_steps_per_s"], 2)
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
    ap.add_argument("--op-time", action="store_true"); ap.add_argument("--wall", action="store_true"); ap.add_argument("--balance", action="store_true")
    ap.add_argument("--calls", type=int, default=50); ap.add_argument("--envs", type=int, default=4096); ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--gradient-steps", type=int, default=1); ap.add_argument("--eval-episodes", type=int, default=64)
    ap.add_argument("--out", default="", help="JSON file to add this mode's section to")
    a = ap.parse_args()
    if a.op_time:
        _emit("op_time", op_time(a.calls), a.out)
    if a.wall:
        _emit("wall", wall(a.envs, a.steps), a.out)
    if a.balance:
        _emit("balance", _run(True, "Env01-v1", a.envs, a.steps, a.gradient_steps, eval_episodes=a.eval_episodes), a.out)


if __name__ == "__main__":
    main()
