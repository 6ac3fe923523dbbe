#!/usr/bin/env python3
"""Microseconds per call of every entry point of the off-policy family (brs_offpolicy.hip, brs_ddpg_learner.hip) with the library that
is loaded, for A/B runs of two builds: one process per build (BRS_HIP_LIB names the other build's library), the processes alternating,
then --summarise over what they wrote (profiles/offpolicy_family_refactor_kernel_times.json).  The method is
tools/td3_kernel_time.py's: a warm-up of 10, three repeats of --calls, the wall clock around the enqueues and one synchronize; the sizes
are the ones DESIGN.md 7.5-7.12 quote: 16,384 envs for act, q and the replay buffer, m = 256 and m = 8,192 for targets and gradients.

    BRS_HIP_LIB=/path/libbrs_hip.so python tools/offpolicy_family_time.py --label parent --out a1.json
    python tools/offpolicy_family_time.py --summarise OUT.json --new new1.json new2.json .. --parent a1.json .. --parent-again b1.json ..

--summarise: per call the median and range of every side over all repeats of all its processes, and the verdict of the issue's rule:
as fast if the new median lies within the spread of the two copies of the parent, or the ranges of new and parent overlap; `by` says
which of the two it was.
"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_ENVS, SIZES, GAMMA = 16384, (256, 8192), 0.99


def measure(calls):
    import torch
    from balance_robot_mujoco_rl_amd import DeviceDDPGLearner, DeviceDDPGNets, DeviceSACLearner, DeviceSACNets, DeviceTD3Learner
    from balance_robot_mujoco_rl_amd.offpolicy import DeviceReplayBuffer, NACTOR, NCRITIC
    from balance_robot_mujoco_rl_amd.nets import ARCHS
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    rand = lambda *s: torch.rand(s, generator=gen, device=dev) * 2 - 1
    w = lambda n: rand(n) * 0.05
    sides = {}
    ddpg, sac = DeviceDDPGNets(device=0), {k: DeviceSACNets(device=0, net_arch=k) for k in ARCHS}
    actor, critic, critics = w(NACTOR), w(NCRITIC), w(2 * NCRITIC)
    sac_w = {k: (w(a.nactor + 1), w(2 * a.ncritic)) for k, a in ARCHS.items()}
    obs, act, out = rand(N_ENVS, 6), rand(N_ENVS, 2), torch.empty((N_ENVS, 2), device=dev)
    q_out = torch.empty(N_ENVS, device=dev)
    sides["ddpg_act"] = lambda k: ddpg.act(actor, obs, k, 0.1, out=out)
    sides["ddpg_act_random"] = lambda k: ddpg.act(None, None, k, 0.1, random=True, out=out)
    sides["ddpg_q"] = lambda k: ddpg.q(critic, obs, act, out=q_out)
    for name, nets in sac.items():
        a, c = sac_w[name]
        sides[f"sac_act/{name}"] = lambda k, nets=nets, a=a: nets.act(a, obs, k, out=out)
        sides[f"sac_q/{name}"] = lambda k, nets=nets, c=c: nets.q(c[:c.numel() // 2], obs, act, out=q_out)
    sides["sac_act_random"] = lambda k: sac["reference"].act(None, None, k, random=True, out=out)
    buf = DeviceReplayBuffer(N_ENVS, 8, device=0)
    flags = (torch.arange(N_ENVS, device=dev) % 5 == 0).to(torch.uint8)
    sides["replay_add"] = lambda k: buf.add(obs, act, obs, obs, q_out, flags, flags)
    batch = buf.new_batch(256)
    sides["replay_sample"] = lambda k: buf.sample(256, out=batch)
    keep = []
    for m in SIZES:
        o, a, y, r = rand(m, 6), rand(m, 2), rand(m), rand(m)
        done, y_out = (torch.arange(m, device=dev) % 3 == 1).to(torch.uint8), torch.empty(m, device=dev)
        one, twin = DeviceDDPGLearner(device=0, max_batch=m), DeviceTD3Learner(device=0, max_batch=m)
        keep += [one, twin]
        sides[f"ddpg_td_target/m{m}"] = lambda k, o=o, r=r, done=done, y_out=y_out: ddpg.td_target(actor, critic, o, r, done, GAMMA, out=y_out)
        sides[f"td3_td_target/m{m}"] = lambda k, o=o, r=r, done=done, y_out=y_out: ddpg.td3_target(actor, critics, o, r, done, GAMMA, 0.2, 0.5, k, out=y_out)
        sides[f"critic_grad/m{m}"] = lambda k, one=one, o=o, a=a, y=y: one.critic_grad(critic, o, a, y)
        sides[f"twin_critic_grad/m{m}"] = lambda k, twin=twin, o=o, a=a, y=y: twin.twin_critic_grad(critics, o, a, y)
        sides[f"actor_grad/m{m}"] = lambda k, one=one, o=o: one.actor_grad(actor, critic, o)
        for name in ARCHS:
            pi, qf = sac_w[name]
            lrn = DeviceSACLearner(device=0, max_batch=m, net_arch=name)
            keep.append(lrn)
            sides[f"sac_td_target/{name}/m{m}"] = lambda k, n=sac[name], pi=pi, qf=qf, o=o, r=r, done=done, y_out=y_out: n.sac_target(pi, qf, o, r, done, GAMMA, k, out=y_out)
            sides[f"sac_twin_critic_grad/{name}/m{m}"] = lambda k, lrn=lrn, qf=qf, o=o, a=a, y=y: lrn.twin_critic_grad(qf, o, a, y)
            sides[f"sac_actor_grad/{name}/m{m}"] = lambda k, lrn=lrn, pi=pi, qf=qf, o=o: lrn.actor_grad(pi, qf, o, k)
    params, target = critics.clone(), critics.clone()
    sides["apply"] = lambda k: keep[1].apply_critics(params, target)
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
            t[name].append(round((time.perf_counter() - t0) / calls * 1e6, 2))
    return t


def summarise(out, new, parent, again):
    load = lambda files: [json.load(open(f)) for f in files]
    docs = {"new": load(new), "parent": load(parent), "parent_again": load(again)}
    res = {"units": "microseconds per call (every kernel the call launches)", "calls_per_repeat": docs["new"][0]["calls"], "repeats_per_process": 3,
           "processes_per_side": len(new), "order": "parent, new, parent_again, repeated", "build_ids": {k: v[0]["build_id"] for k, v in docs.items()},
           "rule": "as fast if the new median is within the spread of the two parent medians around the parent's, or the ranges overlap", "calls": {}}
    for name in docs["new"][0]["us"]:
        us = {k: [x for d in v for x in d["us"][name]] for k, v in docs.items()}
        med = {k: statistics.median(v) for k, v in us.items()}
        spread = abs(med["parent"] - med["parent_again"])
        overlap = min(us["new"]) <= max(us["parent"] + us["parent_again"]) and max(us["new"]) >= min(us["parent"] + us["parent_again"])
        by_median = med["new"] <= max(med["parent"], med["parent_again"]) + spread
        res["calls"][name] = {**{k + "_us": v for k, v in us.items()}, **{k + "_median_us": round(m, 2) for k, m in med.items()},
                              "parent_spread_us": round(spread, 2), "as_fast": bool(by_median or overlap),
                              "by": "median" if by_median else "overlapping ranges only" if overlap else "neither"}
    json.dump(res, open(out, "w"), indent=1)
    for by in ("overlapping ranges only", "neither"):
        print(f"{out}: {len(res['calls'])} calls, {by}: {[k for k, v in res['calls'].items() if v['by'] == by]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="new"); ap.add_argument("--calls", type=int, default=200); ap.add_argument("--out", default="")
    ap.add_argument("--summarise", default=""); ap.add_argument("--new", nargs="*"); ap.add_argument("--parent", nargs="*"); ap.add_argument("--parent-again", nargs="*")
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise, a.new, a.parent, a.parent_again)
    from balance_robot_mujoco_rl_amd import _lib
    doc = {"label": a.label, "build_id": _lib.build_id(), "library": os.environ.get("BRS_HIP_LIB", "in tree"), "calls": a.calls, "us": measure(a.calls)}
    if a.out:
        json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps({k: statistics.median(v) for k, v in doc["us"].items()}))


if __name__ == "__main__":
    main()
