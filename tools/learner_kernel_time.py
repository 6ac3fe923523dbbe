#!/usr/bin/env python3
"""What the device learner costs, three measurements that end up in profiles/learner_kernel_stats.json (each mode
adds its section to --out):

  step time       profiler off: seconds per optimiser step of the torch path (the minibatch body of tools/train_ppo_torch.py::train,
                  restated below on the ActorCritic of --tools-dir) and of DevicePPOLearner.step, minibatches of 8,192 and 65,536
                  rows drawn from a 1 M-row buffer; the two alternate, three repeats each, median over the repeats of the mean of
                  --steps steps after a warm-up
      python3 tools/learner_kernel_time.py --step-time [--tools-dir DIR] --out profiles/learner_kernel_stats.json
  kernel times    the learner's four kernels under the profiler (no other tracing, no counters)
      rocprofv3 --kernel-trace --stats -f csv -d OUT -o lrn -- python3 tools/learner_kernel_time.py
      python3 tools/learner_kernel_time.py --summarise OUT --out profiles/learner_kernel_stats.json
  stage-1 wall    the recipe of tests/test_ppo_device_rollout.py (16,384 Env01-v2 envs, 80 x 64 steps, 4 epochs, minibatch 8,192)
                  with torch's gradient step and with the device learner
      python3 tools/learner_kernel_time.py --stage1 [--iters 80] --out profiles/learner_kernel_stats.json
"""
import argparse, csv, glob, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNELS = ("learner_adv_kernel", "learner_grad_kernel", "learner_reduce_kernel", "learner_apply_kernel")
ROWS = 1 << 20


def summarise(out_dir, m):
    """-> dict from the *_kernel_trace.csv of a rocprofv3 run: per kernel the calls and the mean / median / min duration"""
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no *kernel_trace.csv under {out_dir}"
    dur, names = {k: [] for k in KERNELS}, {}
    for row in csv.DictReader(open(files[0])):
        name = row["Kernel_Name"]
        key = next((k for k in KERNELS if k in name), None)
        if key:
            dur[key].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1000.0)
            names.setdefault(key, name[:120])
    res = {"command": f"rocprofv3 --kernel-trace --stats -f csv -- python3 tools/learner_kernel_time.py --m {m}", "minibatch": m, "rows": ROWS,
           "units": "microseconds", "kernels": {}}
    for k, d in dur.items():
        d = sorted(d)
        if d:
            res["kernels"][k] = dict(name=names[k], calls=len(d), mean_us=round(sum(d) / len(d), 3), median_us=round(d[len(d) // 2], 3),
                                     min_us=round(d[0], 3), max_us=round(d[-1], 3))
    res["sum_of_medians_us"] = round(sum(v["median_us"] for v in res["kernels"].values()), 3)
    return res


def _buffer(torch, T, seed=0):
    """a 1 M-row rollout of the sizes and scales the envs produce, from a freshly initialised ActorCritic"""
    torch.manual_seed(seed)
    model = T.ActorCritic(-0.5).to("cuda")
    obs = (torch.randn(ROWS, 6, device="cuda") * torch.tensor([0.3, 2, 5, 5, 3, 3], device="cuda")).contiguous()
    with torch.no_grad():
        d = model.dist(obs)
        act = d.sample()
        logp = (d.log_prob(act).sum(-1) + 0.1 * torch.randn(ROWS, device="cuda")).contiguous()
    return model, dict(obs=obs, act=act.contiguous(), logp=logp, adv=torch.randn(ROWS, device="cuda"), ret=3 * torch.randn(ROWS, device="cuda"))


def torch_step(torch, nn, model, opt, B, idx, clip=0.2, ent=0.0):
    """tools/train_ppo_torch.py::train, the body of the minibatch loop (no target_kl, no warm-up, one rank)"""
    d = model.dist(B["obs"][idx])
    logp = d.log_prob(B["act"][idx]).sum(-1)
    lr_ = logp - B["logp"][idx]
    ratio = lr_.exp()
    a_ = B["adv"][idx]; a_ = (a_ - a_.mean()) / (a_.std() + 1e-8)
    pl = -torch.min(ratio * a_, ratio.clamp(1 - clip, 1 + clip) * a_).mean()
    vl = 0.5 * (model.v(B["obs"][idx]).squeeze(-1) - B["ret"][idx] / model.ret_scale).pow(2).mean()
    loss = pl + 0.5 * vl - ent * d.entropy().sum(-1).mean()
    opt.zero_grad(set_to_none=True); loss.backward()
    nn.utils.clip_grad_norm_(list(model.pi.parameters()) + [model.log_std], 0.5)
    nn.utils.clip_grad_norm_(model.v.parameters(), 0.5); opt.step()


def step_time(tools_dir, steps, sizes):
    import torch
    import torch.nn as nn
    sys.path.insert(0, tools_dir)
    import train_ppo_torch as T
    from balance_robot_mujoco_rl_amd import DevicePPOLearner
    model, B = _buffer(torch, T)
    opt = torch.optim.Adam(model.parameters(), lr=3e-4)
    lrn = DevicePPOLearner(device=0, vf_coef=0.5, max_grad_norm=0.5, separate_clip=True).load(model.state_dict())
    import hashlib
    res = {"train_ppo_torch_sha256": hashlib.sha256(open(T.__file__, "rb").read()).hexdigest()[:16], "rows": ROWS, "steps_per_repeat": steps, "repeats": 3, "units": "microseconds per optimiser step",
           "sizes": {}}
    for m in sizes:
        perm = torch.randperm(ROWS, device="cuda")
        idx64 = [perm[(k * m) % (ROWS - m):][:m] for k in range(8)]
        idx32 = [i.to(torch.int32).contiguous() for i in idx64]
        sides = {"torch": lambda k: torch_step(torch, nn, model, opt, B, idx64[k % 8]),
                 "device": lambda k: lrn.step(B["obs"], B["act"], B["logp"], B["adv"], B["ret"], idx32[k % 8])}
        for f in sides.values():   # warm-up: library load, first launches, allocator
            for k in range(20):
                f(k)
        torch.cuda.synchronize()
        t = {k: [] for k in sides}
        for _ in range(3):
            for name, f in sides.items():   # alternating, so that both see the same clocks
                t0 = time.perf_counter()
                for k in range(steps):
                    f(k)
                torch.cuda.synchronize()
                t[name].append((time.perf_counter() - t0) / steps * 1e6)
        med = {k: statistics.median(v) for k, v in t.items()}
        res["sizes"][str(m)] = dict(torch_us=[round(x, 2) for x in t["torch"]], device_us=[round(x, 2) for x in t["device"]],
                                    torch_median_us=round(med["torch"], 2), device_median_us=round(med["device"], 2),
                                    torch_over_device=round(med["torch"] / med["device"], 2))
    s = lrn.stats()
    res["device_learner_state"] = dict(steps=s.steps, bad_index=s.bad_index, approx_kl=s.approx_kl)
    return res


def stage1(iters):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_ppo_torch as T
    from balance_robot_mujoco_rl_amd import BatchedSim
    res = {"recipe": f"Env01-v2, 16384 envs, {iters} iterations x 64 steps, 4 epochs, minibatch 8192 (tests/test_ppo_device_rollout.py)", "runs": []}
    for device_learner in (False, True):
        torch.manual_seed(0)
        model = T.ActorCritic(-0.5).to("cuda")
        with torch.no_grad():
            sc = torch.tensor([1, 0.02, 1, 1, 1, 1], device="cuda")
            model.pi[0].weight.mul_(sc); model.v[0].weight.mul_(sc)
        torch.manual_seed(1000)
        opt = torch.optim.Adam(model.parameters(), lr=3e-4)
        sim = BatchedSim("Env01-v2", 16384, device=0, seed=0, auto_reset=True)
        log = []
        torch.cuda.synchronize(); t0 = time.perf_counter()
        T.train(sim, model, opt, iters=iters, n_steps=64, epochs=4, minibatch=8192, gamma=0.999, lam=0.95, clip=0.2, log=log, tag="Env01-v2",
                reward_clip=1.0, device_rollout=True, seed=1000, device_learner=device_learner)
        torch.cuda.synchronize(); wall = time.perf_counter() - t0
        sim.close()
        ev = T.evaluate("Env01-v2", model, 2048, 600)
        res["runs"].append(dict(device_learner=device_learner, wall_s=round(wall, 2), env_steps=log[-1]["env_steps"],
                                env_steps_per_s=round(log[-1]["env_steps"] / wall), updates_last_iter=log[-1]["updates"],
                                still_up_after_600_steps_of_2048=ev["first_episode_still_running"]))
    res["torch_over_device_wall"] = round(res["runs"][0]["wall_s"] / res["runs"][1]["wall_s"], 2)
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
    ap.add_argument("--m", type=int, default=8192); ap.add_argument("--steps", type=int, default=200); ap.add_argument("--iters", type=int, default=80)
    ap.add_argument("--summarise"); ap.add_argument("--step-time", action="store_true"); ap.add_argument("--stage1", action="store_true")
    ap.add_argument("--tools-dir", default=os.path.join(ROOT, "tools"), help="--step-time: the directory train_ppo_torch.py is taken from")
    ap.add_argument("--out", default="", help="JSON file to add this mode's section to")
    a = ap.parse_args()
    if a.summarise:
        return _emit(f"kernel_trace_m{a.m}", summarise(a.summarise, a.m), a.out)
    if a.step_time:
        return _emit("step_time", step_time(os.path.abspath(a.tools_dir), a.steps, (8192, 65536)), a.out)
    if a.stage1:
        return _emit("stage1_wall", stage1(a.iters), a.out)
    # the run the profiler watches
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_ppo_torch as T
    from balance_robot_mujoco_rl_amd import DevicePPOLearner
    model, B = _buffer(torch, T)
    lrn = DevicePPOLearner(device=0, vf_coef=0.5, max_grad_norm=0.5, separate_clip=True).load(model.state_dict())
    idx = torch.randperm(ROWS, device="cuda")[:a.m].to(torch.int32).contiguous()
    for _ in range(a.steps):
        lrn.step(B["obs"], B["act"], B["logp"], B["adv"], B["ret"], idx)
    torch.cuda.synchronize()
    s = lrn.stats()
    print(json.dumps(dict(minibatch=a.m, steps=s.steps, approx_kl=s.approx_kl, bad_index=s.bad_index)))


if __name__ == "__main__":
    main()
