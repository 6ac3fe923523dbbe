#!/usr/bin/env python3
"""Kernel time of the int8 actor next to the float policy kernel, in ONE run: both evaluate the reference's
shipped policy on the same 65,536 observations, `--calls` times each.  Run it under the profiler, then condense the trace:

    rocprofv3 --kernel-trace --stats -f csv -d OUT -o qp -- python3 tools/qpolicy_kernel_time.py
    python3 tools/qpolicy_kernel_time.py --summarise OUT > profiles/qpolicy_kernel_stats.json

The float kernel (policy_act_kernel, deterministic) evaluates two towers (actor and critic), the int8 kernel one."""
import argparse, csv, glob, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNELS = ("qpolicy_act_kernel", "policy_act_kernel")


def summarise(out_dir, envs, calls):
    """-> dict from the *_kernel_trace.csv of a rocprofv3 run: per kernel the calls and the mean / median / min duration"""
    from balance_robot_mujoco_rl_amd import _lib
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no *kernel_trace.csv under {out_dir}"
    dur = {k: [] for k in KERNELS}
    for row in csv.DictReader(open(files[0])):
        name = row["Kernel_Name"]
        key = next((k for k in KERNELS if ("::" + k + "(") in name or name.startswith(k)), None)
        if key:
            dur[key].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1000.0)
    res = {"command": f"rocprofv3 --kernel-trace --stats -f csv -- python3 tools/qpolicy_kernel_time.py --envs {envs} --calls {calls}",
           "build_id": _lib.build_id(), "envs": envs, "units": "microseconds", "kernels": {}}
    for k, d in dur.items():
        d = sorted(d)
        res["kernels"][k] = dict(calls=len(d), mean_us=round(sum(d) / len(d), 3), median_us=round(d[len(d) // 2], 3), min_us=round(d[0], 3))
    res["int8_over_float"] = round(res["kernels"][KERNELS[0]]["median_us"] / res["kernels"][KERNELS[1]]["median_us"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536); ap.add_argument("--calls", type=int, default=50); ap.add_argument("--summarise")
    a = ap.parse_args()
    if a.summarise:
        print(json.dumps(summarise(a.summarise, a.envs, a.calls), indent=1))
        return
    import torch
    from balance_robot_mujoco_rl_amd import BatchedSim, QuantModel, QuantPolicy
    from balance_robot_mujoco_rl_amd.policy import DevicePolicy
    qm = QuantModel.load(os.path.join(ROOT, "tests", "golden", "robot_move_policy.npz"), "mean")
    qpol, fpol = QuantPolicy(qm, device=0), DevicePolicy(device=0)
    fpol.set_weights(qm.float_params())
    sim = BatchedSim("Env01-v3", a.envs, device=0, seed=1, auto_reset=True)
    obs = sim.reset()
    for _ in range(20):  # observations of robots that are being driven, not the reset pose
        obs = sim.step(qpol.act(obs))[0]
    out_f = fpol.act(obs, 0, deterministic=True)
    out_q, codes = qpol.act(obs), torch.empty((a.envs, 2), dtype=torch.int8, device=obs.device)
    for t in range(a.calls):  # alternate, so that both kernels see the same clocks
        fpol.act(obs, t, deterministic=True, out=out_f)
        qpol.act(obs, out=out_q, out_q=codes)
    torch.cuda.synchronize()
    print(json.dumps(dict(envs=a.envs, calls=a.calls, max_abs_difference_of_the_outputs=float((out_f[0] - out_q).abs().max()))))


if __name__ == "__main__":
    main()
