#!/usr/bin/env python3
"""What the episode monitor costs, three measurements that end up in profiles/monitor_kernel_stats.json:

  kernel times    DeviceRollout.collect() with a monitor on 65,536 Env03-v2 envs under the profiler: monitor_update_kernel and
                  monitor_reduce_kernel next to the bootstrap kernel (the yardstick: it reads the same arrays) and the step kernel
                  of the same trace
      rocprofv3 --kernel-trace --stats -f csv -d OUT -o mon -- python3 tools/monitor_kernel_time.py
      python3 tools/monitor_kernel_time.py --summarise OUT > kernels.json
  collect() rate  profiler off: env-steps/s of collect() with and without a monitor, alternating, three repeats each
      python3 tools/monitor_kernel_time.py --rate > rate.json
  evaluate() wall time of tools/train_ppo_torch.py::evaluate (Env01-v2, 4,096 envs, 600 steps; run it on the parent commit's
                  tools/ too, in the same call, for the comparison)
      python3 tools/monitor_kernel_time.py --evaluate [--tools-dir DIR] > evaluate.json
"""
import argparse, csv, glob, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNELS = ("monitor_update_kernel", "monitor_reduce_kernel", "bootstrap_kernel", "brs_step_kernel")


def summarise(out_dir, envs):
    """-> dict from the *_kernel_trace.csv of a rocprofv3 run: per kernel the calls and the mean / median / min duration"""
    from balance_robot_mujoco_rl_amd import _lib
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no *kernel_trace.csv under {out_dir}"
    dur, names = {k: [] for k in KERNELS}, {}
    for row in csv.DictReader(open(files[0])):
        name = row["Kernel_Name"]
        key = next((k for k in KERNELS if k in name), None)
        if key:
            dur[key].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1000.0)
            names.setdefault(key, name[:120])
    res = {"command": f"rocprofv3 --kernel-trace --stats -f csv -- python3 tools/monitor_kernel_time.py --envs {envs}",
           "build_id": _lib.build_id(), "env": "Env03-v2", "envs": envs, "units": "microseconds", "kernels": {}}
    for k, d in dur.items():
        d = sorted(d)
        if d:
            res["kernels"][k] = dict(name=names[k], calls=len(d), mean_us=round(sum(d) / len(d), 3), median_us=round(d[len(d) // 2], 3),
                                     min_us=round(d[0], 3), max_us=round(d[-1], 3))
    if "bootstrap_kernel" in res["kernels"] and "monitor_update_kernel" in res["kernels"]:
        res["update_over_bootstrap"] = round(res["kernels"]["monitor_update_kernel"]["median_us"] / res["kernels"]["bootstrap_kernel"]["median_us"], 3)
    return res


def _rollout(envs, T, monitor):
    import numpy as np
    from balance_robot_mujoco_rl_amd import BatchedSim, EpisodeMonitor
    from balance_robot_mujoco_rl_amd.policy import DevicePolicy, DeviceRollout, NPARAM
    sim = BatchedSim("Env03-v2", envs, device=0, seed=0, auto_reset=True)
    pol = DevicePolicy(device=0, seed=1)
    w = (np.random.default_rng(0).standard_normal(NPARAM) * 0.1).astype(np.float32); w[-2:] = 0.0
    pol.set_weights(w)
    mon = EpisodeMonitor(envs, device=0) if monitor else None
    return DeviceRollout(sim, pol, T, monitor=mon), mon


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536); ap.add_argument("--T", type=int, default=32); ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--summarise"); ap.add_argument("--rate", action="store_true"); ap.add_argument("--evaluate", action="store_true")
    ap.add_argument("--tools-dir", default=os.path.join(ROOT, "tools"), help="--evaluate: the directory train_ppo_torch.py is taken from")
    a = ap.parse_args()
    if a.summarise:
        print(json.dumps(summarise(a.summarise, a.envs), indent=1))
        return
    import torch
    if a.evaluate:
        sys.path.insert(0, a.tools_dir)
        import train_ppo_torch as T
        torch.manual_seed(0)
        model = T.ActorCritic(-0.5).to("cuda")
        T.evaluate("Env01-v2", model, 256, 20)   # warm-up: library load, first launches
        torch.cuda.synchronize()
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            res = T.evaluate("Env01-v2", model, 4096, 600)
            torch.cuda.synchronize()
            walls.append(round(time.perf_counter() - t0, 4))
        print(json.dumps(dict(tools_dir=a.tools_dir, env="Env01-v2", envs=4096, steps=600, wall_s=walls, result=res)))
        return
    if a.rate:
        ros = {False: _rollout(a.envs, a.T, False)[0], True: _rollout(a.envs, a.T, True)[0]}
        rates = {False: [], True: []}
        for ro in ros.values():
            ro.collect()   # warm-up; also the reset
        torch.cuda.synchronize()
        for _ in range(3):
            for with_monitor in (False, True):   # alternating, so that both see the same clocks
                t0 = time.perf_counter()
                for _ in range(a.rounds):
                    ros[with_monitor].collect()
                torch.cuda.synchronize()
                rates[with_monitor].append(a.envs * a.T * a.rounds / (time.perf_counter() - t0))
        wo, wi = rates[False], rates[True]
        print(json.dumps(dict(env="Env03-v2", envs=a.envs, rollout_steps=a.T, rounds=a.rounds, without_monitor_env_steps_per_s=wo,
                              with_monitor_env_steps_per_s=wi, spread_without=(max(wo) - min(wo)) / (sum(wo) / 3),
                              cost_of_monitor=1 - (sum(wi) / 3) / (sum(wo) / 3), stats=dataclass_dict(ros[True].monitor.stats()))))
        return
    ro, mon = _rollout(a.envs, a.T, True)
    for _ in range(a.rounds):
        ro.collect()
        s = mon.stats()   # one reduce per round
    torch.cuda.synchronize()
    print(json.dumps(dict(envs=a.envs, rollout_steps=a.T, rounds=a.rounds, stats=dataclass_dict(s))))


def dataclass_dict(s):
    import dataclasses
    return dataclasses.asdict(s)


if __name__ == "__main__":
    main()
