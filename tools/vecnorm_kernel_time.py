#!/usr/bin/env python3
"""What VecNormalize on the device costs, two measurements that end up in profiles/vecnorm_kernel_stats.json as its
`step` and `collect` entries:

  step time     microseconds per DeviceVecNormalize.step call, training and frozen, at 16,384, 65,536 and 524,288 envs, next to a
                torch restatement of the same step in fp64 on the device (what a user would write without the kernels; no
                synchronisation in it either), in one process, alternating: warm-up 10 calls, then three repeats of 200 calls
                each, a host clock around calls that end in a device synchronise, profiler off
      python3 tools/vecnorm_kernel_time.py [--out FILE]
  collect()     wall time of DeviceRollout.collect() with and without a normaliser (Env01-v2, 16,384 envs, five steps: the A2C
                configuration of DESIGN.md 7.9), alternating, three repeats
      python3 tools/vecnorm_kernel_time.py --collect
  replay sample the normalising replay sample of DESIGN.md 7.14 -> profiles/vecnorm_replay_kernel_time.json: microseconds per
                minibatch of 256 and of 4,096 from a buffer of 16,384 envs, three variants in one process, alternating, with the
                step time's warm-up, calls and repeats: the plain sample (one launch), the plain sample followed by normalize_obs
                twice and normalize_reward (four launches, what the parent can do), and sample(normalize=) (one launch).  The
                required relation: the slowest repeat of the fused call is not slower than the fastest of the four composed calls.
      python3 tools/vecnorm_kernel_time.py --replay [--out FILE]
"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (16384, 65536, 524288)


class TorchVecNormalize:
    """the step of DESIGN.md 7.13 in torch ops, fp64 on the device; the counts live on the host, nothing synchronises"""

    def __init__(self, n, device, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8):
        import torch
        f = dict(dtype=torch.float64, device=device)
        self.mean, self.var, self.count = torch.zeros(6, **f), torch.ones(6, **f), 1e-4
        self.ret_mean, self.ret_var, self.ret_count = torch.zeros((), **f), torch.ones((), **f), 1e-4
        self.returns = torch.zeros(n, **f)
        self.clip_obs, self.clip_reward, self.gamma, self.epsilon, self.training = clip_obs, clip_reward, gamma, epsilon, True

    @staticmethod
    def _update(mean, var, count, x):
        n = x.shape[0]
        bm, bv = x.mean(0), x.var(0, unbiased=False)
        delta, tot = bm - mean, count + n
        m2 = var * count + bv * n + delta * delta * count * n / tot
        return mean + delta * n / tot, m2 / tot, tot

    def step(self, obs, reward, terminated, truncated, terminal_obs):
        import torch
        if self.training:
            self.mean, self.var, self.count = self._update(self.mean, self.var, self.count, obs.double())
            self.returns = self.returns * self.gamma + reward.double()
            self.ret_mean, self.ret_var, self.ret_count = self._update(self.ret_mean, self.ret_var, self.ret_count, self.returns)
        sd = torch.sqrt(self.var + self.epsilon)
        o = ((obs.double() - self.mean) / sd).clamp(-self.clip_obs, self.clip_obs).float()
        t = ((terminal_obs.double() - self.mean) / sd).clamp(-self.clip_obs, self.clip_obs).float()
        r = (reward.double() / torch.sqrt(self.ret_var + self.epsilon)).clamp(-self.clip_reward, self.clip_reward).float()
        self.returns.masked_fill_((terminated | truncated).bool(), 0.0)
        return o, r, t


def _inputs(n, dev):
    import torch
    g = torch.Generator(device=dev).manual_seed(n)
    scale = torch.tensor([0.1, 10.0, 3.0, 0.25, 2.0, 1.0], device=dev)
    mk = lambda: torch.randn((n, 6), device=dev, generator=g) * scale + 0.5
    return (mk(), 1.0 + 0.2 * torch.randn(n, device=dev, generator=g), (torch.rand(n, device=dev, generator=g) < 0.01).to(torch.uint8),
            (torch.rand(n, device=dev, generator=g) < 0.005).to(torch.uint8), mk())


def step_times(warmup, calls, repeats):
    import torch
    from balance_robot_mujoco_rl_amd import DeviceVecNormalize, _lib
    dev = torch.device("cuda", 0)
    res = dict(command="python3 tools/vecnorm_kernel_time.py", build_id=_lib.build_id(), units="microseconds per step call",
               warmup=warmup, calls=calls, repeats=repeats, sizes={})
    for n in SIZES:
        ins = _inputs(n, dev)
        impl = {"kernels": DeviceVecNormalize(n, device=0), "torch_fp64": TorchVecNormalize(n, dev)}
        for v in impl.values():
            for training in (True, False):
                v.training = training
                for _ in range(warmup):
                    v.step(*ins)
        torch.cuda.synchronize()
        us = {(k, tr): [] for k in impl for tr in (True, False)}
        for _ in range(repeats):
            for training in (True, False):
                for k, v in impl.items():   # alternating, so that both see the same clocks
                    v.training = training
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        out = v.step(*ins)
                    torch.cuda.synchronize()
                    us[(k, training)].append(round((time.perf_counter() - t0) / calls * 1e6, 2))
        # both saw the same batches the same number of times: the outputs agree to fp32 rounding
        a, b = impl["kernels"].step(*ins), impl["torch_fp64"].step(*ins)
        diff = max(float((x - y).abs().max()) for x, y in zip(a, b))
        row = dict(max_abs_output_difference=diff)
        for training in (True, False):
            k, t = us[("kernels", training)], us[("torch_fp64", training)]
            row["training" if training else "frozen"] = dict(kernels_us=k, torch_fp64_us=t, torch_over_kernels=round(min(t) / min(k), 2),
                                                             slowest_kernels_over_fastest_torch=round(max(k) / min(t), 3))
        res["sizes"][str(n)] = row
        impl["kernels"].close()
        del out
    return res


def collect_times(envs, T, rounds, repeats):
    import numpy as np
    import torch
    from balance_robot_mujoco_rl_amd import BatchedSim, DeviceVecNormalize, EpisodeMonitor, _lib
    from balance_robot_mujoco_rl_amd.policy import DevicePolicy, DeviceRollout, NPARAM
    ros = {}
    for with_norm in (False, True):
        sim = BatchedSim("Env01-v2", envs, device=0, seed=0, auto_reset=True)
        pol = DevicePolicy(device=0, seed=1)
        w = (np.random.default_rng(0).standard_normal(NPARAM) * 0.1).astype(np.float32); w[-2:] = 0.0
        pol.set_weights(w)
        ros[with_norm] = DeviceRollout(sim, pol, T, gae_lambda=1.0, monitor=EpisodeMonitor(envs, device=0),
                                       normalize=DeviceVecNormalize(envs, device=0) if with_norm else None)
    for ro in ros.values():
        for _ in range(3):
            ro.collect()
    torch.cuda.synchronize()
    ms = {False: [], True: []}
    for _ in range(repeats):
        for with_norm in (False, True):
            t0 = time.perf_counter()
            for _ in range(rounds):
                ros[with_norm].collect()
            torch.cuda.synchronize()
            ms[with_norm].append(round((time.perf_counter() - t0) / rounds * 1e3, 4))
    return dict(command="python3 tools/vecnorm_kernel_time.py --collect", build_id=_lib.build_id(), env="Env01-v2", envs=envs, rollout_steps=T,
                rounds=rounds, units="milliseconds per collect()", without_normaliser_ms=ms[False], with_normaliser_ms=ms[True],
                added_share=round(min(ms[True]) / min(ms[False]) - 1, 4))


def replay_times(envs, cap, warmup, calls, repeats, batches=(256, 4096)):
    import torch
    from balance_robot_mujoco_rl_amd import DeviceReplayBuffer, DeviceVecNormalize, _lib
    dev = torch.device("cuda", 0)
    rb, norm = DeviceReplayBuffer(envs, cap, device=0, seed=3), DeviceVecNormalize(envs, device=0)
    norm.reset(_inputs(envs, dev)[0])
    last = _inputs(envs, dev)[0]
    for t in range(cap):   # a full buffer of raw transitions, the statistics trained on them
        obs, rew, te, tr, tobs = _inputs(envs + t + 1, dev)
        obs, tobs = obs[:envs].contiguous(), tobs[:envs].contiguous()
        rew, te, tr = rew[:envs].contiguous(), te[:envs].contiguous(), tr[:envs].contiguous()
        norm.step(obs, rew, te, tr, tobs)
        rb.add(last, torch.zeros((envs, 2), device=dev), obs, tobs, rew, te, tr)
        last = obs
    res = dict(command="python3 tools/vecnorm_kernel_time.py --replay", build_id=_lib.build_id(), units="microseconds per minibatch",
               envs=envs, capacity_steps=cap, warmup=warmup, calls=calls, repeats=repeats, batches={})
    for m in batches:
        out, tmp = rb.new_batch(m), rb.new_batch(m)

        def plain():
            rb.sample(m, out=out)

        def composed():
            rb.sample(m, out=tmp)
            norm.normalize_obs(tmp[0], out=out[0]); norm.normalize_obs(tmp[1], out=out[1]); norm.normalize_reward(tmp[3], out=out[3])

        def fused():
            rb.sample(m, out=out, normalize=norm)
        variants = {"plain": plain, "composed": composed, "fused": fused}
        for fn in variants.values():
            for _ in range(warmup):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in variants}
        for _ in range(repeats):
            for k, fn in variants.items():   # alternating, so that all see the same clocks
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn()
                torch.cuda.synchronize()
                us[k].append(round((time.perf_counter() - t0) / calls * 1e6, 2))
        # the same draw through the composed and the fused path: the same bytes
        rb.draw = 7; composed(); a = [t.clone() for t in (out[0], out[1], out[3])]
        rb.draw = 7; fused(); same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, (out[0], out[1], out[3])))
        res["batches"][str(m)] = dict(plain_us=us["plain"], composed_four_calls_us=us["composed"], fused_us=us["fused"],
                                      slowest_fused_over_fastest_composed=round(max(us["fused"]) / min(us["composed"]), 3),
                                      fused_over_plain=round(min(us["fused"]) / min(us["plain"]), 3), fused_equals_composed_bytes=same,
                                      requirement_met=max(us["fused"]) <= min(us["composed"]))
    norm.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replay", action="store_true"); ap.add_argument("--capacity-steps", type=int, default=8)
    ap.add_argument("--collect", action="store_true"); ap.add_argument("--envs", type=int, default=16384); ap.add_argument("--T", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10); ap.add_argument("--calls", type=int, default=200); ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.replay:
        res = replay_times(a.envs, a.capacity_steps, a.warmup, a.calls, a.repeats)
    else:
        res = collect_times(a.envs, a.T, a.rounds, a.repeats) if a.collect else step_times(a.warmup, a.calls, a.repeats)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
