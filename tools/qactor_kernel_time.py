#!/usr/bin/env python3
"""Kernel time of the int8 off-policy actor (qactor_act_kernel) next to the float actor of the same network (ddpg_act_kernel) and
the int8 PPO actor (qpolicy_act_kernel), in ONE run: all three evaluate the same observations, `--calls` times
each at every size of `--envs`, alternating, after `--warmup` calls.  Run it under the profiler, then condense the trace:

    rocprofv3 --kernel-trace --stats -f csv -d OUT -o qa -- python3 tools/qactor_kernel_time.py
    python3 tools/qactor_kernel_time.py --summarise OUT > profiles/qactor_kernel_stats.json

The int8 and float off-policy actors are the same 6-300-200-2 network (the hand-built PD actor of tests/qactor_cases.py and its
quantisation); the int8 PPO actor is the 6-64-64-2 network of tests/golden/robot_move_policy.npz, a 15th of the multiply-adds.

--archs: the two instantiations of the int8 kernel (6-300-200-2 and 6-256-256-2, SB3's SAC default) next to the two of the float
SAC actor (sac_act_kernel, deterministic) instead, the four alternating on the same observations under the same procedure; pass it
to both commands, and write the summary to profiles/qactor_arch_kernel_stats.json.  Each network is the PD actor of its widths."""
import argparse, csv, glob, json, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNELS = ("qactor_act_kernel", "ddpg_act_kernel", "qpolicy_act_kernel")
ARCH_KERNELS = ("qactor_act_kernel<brs::qactor::WidthsReference>", "qactor_act_kernel<brs::qactor::Widths256>",
                "sac_act_kernel<brs::sac::ArchReference>", "sac_act_kernel<brs::sac::ArchSacDefault>")
DRIVE = 20  # env steps before the timed calls: observations of robots that are being driven, not the reset pose


def summarise(out_dir, sizes, calls, warmup, archs=False):
    """-> dict from the *_kernel_trace.csv of a rocprofv3 run: per size and kernel the calls and the median / min / quartiles of
    the duration.  Every kernel runs DRIVE + warmup + calls times per size, size after size: the trace is cut by that count
    and the first DRIVE + warmup calls of every size are left out"""
    from balance_robot_mujoco_rl_amd import _lib
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no *kernel_trace.csv under {out_dir}"
    kernels = ARCH_KERNELS if archs else KERNELS
    # a kernel's name in the trace: after a namespace or at the start, then its arguments -- or, for a template, its parameters
    pattern = {k: re.compile(r"(^|::|\s)" + re.escape(k) + r"[(<]") for k in kernels}
    dur = {k: [] for k in kernels}
    for row in csv.DictReader(open(files[0])):
        name = row["Kernel_Name"]
        key = next((k for k in kernels if pattern[k].search(name)), None)
        if key:
            dur[key].append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1000.0))
    per_size = DRIVE + warmup + calls
    for k in kernels:
        assert len(dur[k]) == per_size * len(sizes), f"{k}: {len(dur[k])} calls in the trace, expected {per_size * len(sizes)}"
        dur[k] = [v for _, v in sorted(dur[k])]
    res = {"command": f"rocprofv3 --kernel-trace --stats -f csv -- python3 tools/qactor_kernel_time.py --envs {' '.join(map(str, sizes))} "
                      f"--calls {calls} --warmup {warmup}" + (" --archs" if archs else ""),
           "build_id": _lib.build_id(), "units": "microseconds", "sizes": {}}
    for i, n in enumerate(sizes):
        per = {}
        for k in kernels:
            d = sorted(dur[k][i * per_size + DRIVE + warmup:(i + 1) * per_size])
            per[k] = dict(calls=len(d), median_us=round(d[len(d) // 2], 3), min_us=round(d[0], 3), p25_us=round(d[len(d) // 4], 3),
                          p75_us=round(d[3 * len(d) // 4], 3), max_us=round(d[-1], 3))
        med = lambda k: per[k]["median_us"]
        if archs:
            per["int8_over_float_reference"] = round(med(kernels[0]) / med(kernels[2]), 3)
            per["int8_over_float_256"] = round(med(kernels[1]) / med(kernels[3]), 3)
            per["int8_256_over_int8_reference"] = round(med(kernels[1]) / med(kernels[0]), 3)
        else:
            per["int8_over_float"] = round(med(kernels[0]) / med(kernels[1]), 3)
        res["sizes"][str(n)] = per
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 65536]); ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20); ap.add_argument("--summarise")
    ap.add_argument("--archs", action="store_true", help="the int8 and the float SAC actor at both width sets instead of the three kernels")
    a = ap.parse_args()
    if a.summarise:
        print(json.dumps(summarise(a.summarise, a.envs, a.calls, a.warmup, a.archs), indent=1))
        return
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from tests import qactor_cases as K
    if a.archs:
        return time_archs(a, torch, K)
    from balance_robot_mujoco_rl_amd import BatchedSim, DeviceDDPGNets, QuantActor, QuantModel, QuantPolicy, quantize_actor
    flat = K.pd_actor_params()
    qact, nets = QuantActor(quantize_actor(flat), device=0), DeviceDDPGNets(device=0)
    qpol = QuantPolicy(QuantModel.load(os.path.join(ROOT, "tests", "golden", "robot_move_policy.npz"), "mean"), device=0)
    params = torch.from_numpy(flat).cuda()
    for n in a.envs:
        sim = BatchedSim("Env01-v1", n, device=0, seed=1, auto_reset=True)
        obs = sim.reset()
        out_q, out_f, out_p = (torch.empty((n, 2), device=obs.device) for _ in range(3))
        codes = torch.empty((n, 2), dtype=torch.int8, device=obs.device)
        for t in range(DRIVE + a.warmup + a.calls):  # alternate, so that the kernels see the same clocks
            nets.act(params, obs, t, 0.0, out=out_f)
            qact.act(obs, out=out_q, out_q=codes)
            qpol.act(obs, out=out_p)
            if t < DRIVE:
                obs = sim.step(out_q)[0]
        torch.cuda.synchronize()
        print(json.dumps(dict(envs=n, calls=a.calls, warmup=a.warmup, max_abs_int8_minus_float=float((out_f - out_q).abs().max()))))
        sim.close()


def time_archs(a, torch, K):
    """--archs: int8 6-300-200-2, int8 6-256-256-2, float SAC at the same two widths (deterministic), alternating"""
    import numpy as np
    from tests import qactor_arch_cases as A
    from balance_robot_mujoco_rl_amd import BatchedSim, DeviceSACNets, QuantActor, quantize_actor
    n01 = K.NACTOR - 402
    flat = K.pd_actor_params()
    sac_ref = np.concatenate([flat[:n01 + 400], np.zeros(400, np.float32), flat[n01 + 400:], np.zeros(3, np.float32)])   # zero log_std head
    sac_256 = A.sac_vector(A.pd_actor_params())
    q_ref, q_256 = QuantActor(quantize_actor(sac_ref, head="sac"), device=0), QuantActor(quantize_actor(sac_256, head="sac", net_arch="sb3"), device=0)
    f_ref, f_256 = DeviceSACNets(device=0), DeviceSACNets(device=0, net_arch="sb3")
    p_ref, p_256 = torch.from_numpy(sac_ref).cuda(), torch.from_numpy(sac_256).cuda()
    for n in a.envs:
        sim = BatchedSim("Env01-v1", n, device=0, seed=1, auto_reset=True)
        obs = sim.reset()
        o_qr, o_q2, o_fr, o_f2 = (torch.empty((n, 2), device=obs.device) for _ in range(4))
        codes = torch.empty((n, 2), dtype=torch.int8, device=obs.device)
        for t in range(DRIVE + a.warmup + a.calls):  # alternate, so that the kernels see the same clocks
            f_ref.act(p_ref, obs, t, deterministic=True, out=o_fr)
            q_ref.act(obs, out=o_qr, out_q=codes)
            f_256.act(p_256, obs, t, deterministic=True, out=o_f2)
            q_256.act(obs, out=o_q2, out_q=codes)
            if t < DRIVE:
                obs = sim.step(o_qr)[0]
        torch.cuda.synchronize()
        print(json.dumps(dict(envs=n, calls=a.calls, warmup=a.warmup, max_abs_int8_minus_float_reference=float((o_fr - o_qr).abs().max()),
                              max_abs_int8_minus_float_256=float((o_f2 - o_q2).abs().max()))))
        sim.close()


if __name__ == "__main__":
    main()
