#!/usr/bin/env python3
"""Cost of rgb_array rendering (include/brs_render.h) on two user-sized workloads, timed with device events after warm-up:

  (a) video path: 1 env at 800 x 800 inside a 65,536-env Env03-v2 handle, as BalanceVecEnv.render() does it: pose fetch
      (brs_get_state of the whole handle, host, synchronous), H2D of the selected qpos row, kernel;
  (b) batched pixels: 4,096 envs at 84 x 84, kernel only (qpos already on the device).

Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (tracing slows the host):
    rocprofv3 --kernel-trace --stats -d DIR -o render --output-format csv -- python tools/render_rate.py --iters 20
    python tools/render_rate.py --kernel-trace DIR/.../render_kernel_trace.csv --out profiles/render_rate.json
"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from balance_robot_mujoco_rl_amd import BatchedSim, _lib  # noqa: E402
from balance_robot_mujoco_rl_amd.sim import make_camera  # noqa: E402

HBM_TBPS = 8.0  # MI355X HBM3E peak (datasheet)


def timed(fn, iters):
    """ms per call: device events around `iters` calls (+ host wall clock, which includes any host-side blocking)"""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters, (time.perf_counter() - t0) * 1e3 / iters


def kernel_us(trace_csv):
    """brs_render_kernel durations from a rocprofv3 kernel_trace.csv, per grid size (one grid size per workload)"""
    import csv
    by = {}
    for r in csv.DictReader(open(trace_csv)):
        if "brs_render_kernel" in r.get("Kernel_Name", ""):
            grid = "x".join(r[c] for c in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z") if c in r) or r.get("Grid_Size", "?")
            by.setdefault(grid, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {g: dict(launches=len(v), median_us=float(np.median(v)), min_us=float(np.min(v))) for g, v in by.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200); ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--kernel-trace", default=None); ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {}
    # (a) video path
    n = 65536
    sim = BatchedSim("Env03-v2", n, device=0, seed=0)
    sim.reset()
    g = torch.Generator(device="cuda").manual_seed(0)
    for _ in range(50):
        sim.step(torch.rand((n, 2), device="cuda", generator=g) * 2 - 1)
    torch.cuda.synchronize()
    frame = lambda: sim.render(env_ids=[0])
    for _ in range(a.warmup):
        frame()
    ev, wall = timed(frame, a.iters)
    t0 = time.perf_counter()
    for _ in range(a.iters):
        sim.get_state()
    fetch = (time.perf_counter() - t0) * 1e3 / a.iters
    out["video_1env_800x800"] = dict(handle_envs=n, ms_per_frame_events=ev, ms_per_frame_wall=wall, ms_pose_fetch_wall=fetch,
                                     bytes_written=800 * 800 * 3, pose_bytes_fetched=n * 16 * 8 + n * 14 * 8 * 2 + n * 8)
    # (b) batched pixels, kernel only
    k, W, H = 4096, 84, 84
    L = _lib.lib()
    q = torch.from_numpy(np.ascontiguousarray(sim.get_state()[0][:k])).cuda()
    rgb = torch.empty((k, H, W, 3), dtype=torch.uint8, device="cuda")
    cam = make_camera(dict(width=W, height=H))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    def batch():
        rc = L.brs_render(0, 3, k, C.c_void_p(q.data_ptr()), C.byref(cam), C.c_void_p(rgb.data_ptr()), None, None, stream)
        assert rc == 0, L.brs_render_last_error()
    for _ in range(a.warmup):
        batch()
    ev, wall = timed(batch, a.iters)
    nbytes = k * H * W * 3
    out["batched_4096env_84x84"] = dict(envs=k, ms_per_launch_events=ev, us_per_frame=ev * 1e3 / k, bytes_written=nbytes,
                                        write_TBps=nbytes / (ev * 1e-3) / 1e12, hbm_share=nbytes / (ev * 1e-3) / 1e12 / HBM_TBPS,
                                        pixels_per_s=k * H * W / (ev * 1e-3))
    if a.kernel_trace:
        out["kernel_us_by_grid"] = kernel_us(a.kernel_trace)
    out["note"] = ("events = device events around the calls (the video path's pose fetch blocks the host in between, so the "
                   "events span it); wall = host clock to a device synchronise; kernel times from the rocprofv3 run, by grid size: "
                   "1-env 800x800 = 2,500 workgroups of 256, 4,096-env 84x84 = 147,456 workgroups of 256")
    print(json.dumps(out))
    if a.out:
        json.dump(out, open(a.out, "w"), indent=1)
    sim.close()


if __name__ == "__main__":
    main()
