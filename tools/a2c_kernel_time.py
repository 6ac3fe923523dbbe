#!/usr/bin/env python3
"""What the A2C update costs -> profiles/a2c_kernel_stats.json, with the build id:

  step time      profiler off: microseconds per update of the torch body (tools/train_a2c_torch.py::torch_update) and of
                 DeviceA2CLearner.step on the same rollout of M = 5 x 16,384 and 5 x 65,536 rows; the two alternate, three repeats
                 of --steps updates each after a warm-up, median over the repeats
  kernel times   one run of the device update alone in a child process under `rocprofv3 --kernel-trace --stats` (no other tracing,
                 no counters): per kernel the calls and the mean / median / min / max duration

    python3 tools/a2c_kernel_time.py [--steps 200] [--no-trace] [--out profiles/a2c_kernel_stats.json]
"""
import argparse, json, os, shutil, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("learner_adv_kernel", "learner_a2c_grad_kernel", "learner_reduce_kernel", "learner_rmsprop_apply_kernel")
SIZES = (5 * 16384, 5 * 65536)


def _rollout(torch, T, m, seed=0):
    """m rows of the sizes and scales the envs produce, from a freshly initialised ActorCritic"""
    torch.manual_seed(seed)
    model = T.ActorCritic(0.0).to("cuda")
    obs = (torch.randn(m, 6, device="cuda") * torch.tensor([0.3, 2, 5, 5, 3, 3], device="cuda")).contiguous()
    with torch.no_grad():
        act = model.dist(obs).sample().contiguous()
    return model, (obs, act, torch.randn(m, device="cuda"), 3 * torch.randn(m, device="cuda"))


def step_time(steps):
    import torch
    import train_a2c_torch as T
    from balance_robot_mujoco_rl_amd import DeviceA2CLearner
    res = {"steps_per_repeat": steps, "repeats": 3, "units": "microseconds per update", "sizes": {}}
    for m in SIZES:
        model, B = _rollout(torch, T, m)
        opt = T.RMSpropTFLike(model.parameters())
        lrn = DeviceA2CLearner(device=0).load(model.state_dict())
        sides = {"torch": lambda: T.torch_update(model, opt, *B), "device": lambda: lrn.step(*B)}
        for f in sides.values():   # warm-up: library load, first launches, allocator
            for _ in range(20):
                f()
        torch.cuda.synchronize()
        t = {k: [] for k in sides}
        for _ in range(3):
            for name, f in sides.items():   # alternating, so that both see the same clocks
                t0 = time.perf_counter()
                for _ in range(steps):
                    f()
                torch.cuda.synchronize()
                t[name].append((time.perf_counter() - t0) / steps * 1e6)
        med = {k: statistics.median(v) for k, v in t.items()}
        s = lrn.stats()
        res["sizes"][str(m)] = dict(torch_us=[round(x, 2) for x in t["torch"]], device_us=[round(x, 2) for x in t["device"]],
                                    torch_median_us=round(med["torch"], 2), device_median_us=round(med["device"], 2),
                                    torch_over_device=round(med["torch"] / med["device"], 2), device_steps=s.steps, bad_index=s.bad_index)
        lrn.close()
    return res


def profiled(m, steps):
    """the run the profiler watches: the device update alone"""
    import torch
    import train_a2c_torch as T
    from balance_robot_mujoco_rl_amd import DeviceA2CLearner
    model, B = _rollout(torch, T, m)
    lrn = DeviceA2CLearner(device=0, normalize_advantage=True).load(model.state_dict())   # with the advantage pre-pass in the trace
    for _ in range(steps):
        lrn.step(*B)
    torch.cuda.synchronize()
    s = lrn.stats()
    print(json.dumps(dict(rows=m, steps=s.steps, bad_index=s.bad_index)))


def kernel_trace(m, steps):
    """-> per-kernel durations from a rocprofv3 child run of `--profiled`"""
    import csv, glob
    out_dir = tempfile.mkdtemp(prefix="a2c_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", out_dir, "-o", "a2c", "--",
               sys.executable, os.path.abspath(__file__), "--profiled", "--m", str(m), "--steps", str(steps)]
        subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
        files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
        assert files, f"no *kernel_trace.csv under {out_dir}"
        dur = {k: [] for k in KERNELS}
        for row in csv.DictReader(open(files[0])):
            key = next((k for k in KERNELS if k in row["Kernel_Name"]), None)
            if key:
                dur[key].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1000.0)
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
    res = {"command": "rocprofv3 --kernel-trace --stats -f csv -- python3 tools/a2c_kernel_time.py --profiled", "rows": m, "normalize_advantage": True,
           "units": "microseconds", "kernels": {}}
    for k, d in dur.items():
        d = sorted(d)
        if d:
            res["kernels"][k] = dict(calls=len(d), mean_us=round(sum(d) / len(d), 3), median_us=round(d[len(d) // 2], 3), min_us=round(d[0], 3),
                                     max_us=round(d[-1], 3))
    res["sum_of_medians_us"] = round(sum(v["median_us"] for v in res["kernels"].values()), 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200); ap.add_argument("--m", type=int, default=SIZES[1])
    ap.add_argument("--profiled", action="store_true", help="internal: the child run under the profiler")
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "a2c_kernel_stats.json"))
    a = ap.parse_args()
    if a.profiled:
        return profiled(a.m, a.steps)
    from balance_robot_mujoco_rl_amd import _lib
    doc = {"build_id": _lib.build_id(), "step_time": step_time(a.steps)}
    if not a.no_trace:
        doc["kernel_trace"] = {str(m): kernel_trace(m, a.steps) for m in SIZES}
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
