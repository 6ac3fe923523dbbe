#!/usr/bin/env python3
"""Diagnostic: per-phase wave cycles of the step kernel (needs a -DBRS_TIMING build; run on the GPU box).
    BRS_EXTRA_HIPCC_FLAGS=-DBRS_TIMING python tools/phase_timing.py [Env03-v2 [OUT_DIR]]
    BRS_HIP_LIB=ab/libbrs_hip_timing.so python tools/phase_timing.py [Env03-v2 [OUT_DIR]]   (prebuilt: tools/ab_build.py timing -DBRS_TIMING)
OUT_DIR: also save the raw per-wave records of the last launch there (wave_records_<env>.npy)"""
import ctypes as C, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from balance_robot_mujoco_rl_amd import _lib
if not os.environ.get("BRS_HIP_LIB"):   # (or point BRS_HIP_LIB at a prebuilt -DBRS_TIMING variant: tools/ab_build.py timing -DBRS_TIMING)
    os.environ.setdefault("BRS_EXTRA_HIPCC_FLAGS", "-DBRS_TIMING")
    _lib.build(force=True)
from balance_robot_mujoco_rl_amd import BatchedSim
env = sys.argv[1] if len(sys.argv) > 1 else "Env03-v2"
out_dir = sys.argv[2] if len(sys.argv) > 2 else None
n = 65536
sim = BatchedSim(env, n, seed=0)
sim.reset()
L = _lib.lib()
buf = (C.c_ulonglong * 16)()
g = torch.Generator(device="cuda"); g.manual_seed(1234)
acts = [torch.rand((n, 2), generator=g, device="cuda") * 2 - 1 for _ in range(16)]
for k in range(60): sim.step(acts[k % 16])
torch.cuda.synchronize(); L.brs_debug_counters(buf)
steps = 60
for k in range(steps): sim.step(acts[k % 16])
torch.cuda.synchronize(); L.brs_debug_counters(buf)
names = ["kin+smooth", "collide robot-floor", "collide block-floor", "collide coupled", "assemble", "cholesky", "passA/verify", "integrate", "whole trip", "trips", "  coupled: torso patch", "  coupled: wheels"]
waves = n // 64
tot = buf[8]
print(f"{env}: trips per wave-step {buf[9] / waves / steps:.1f}")
for i, nm in [(j, names[j]) for j in (0, 1, 2, 3, 10, 11, 4, 5, 6, 7, 8)]:
    print(f"  {nm:22s} {buf[i] / waves / steps:12.0f} cycles/wave-step  {100.0 * buf[i] / tot:5.1f}% of trip time   {buf[i] / max(1, buf[9]):8.0f} cycles/trip")

# load balance: with one wave per SIMD the launch lasts as long as its slowest wave
ratios = []
for k in range(20):
    sim.step(acts[k % 16]); torch.cuda.synchronize(); L.brs_debug_counters(buf)
    mean_c, max_c, mean_t, max_t = buf[8] / waves, buf[12], buf[9] / waves, buf[13]
    ratios.append((max_c / mean_c, max_t / mean_t, mean_t, max_t))
import statistics as st_
print(f"  slowest wave / mean wave: cycles x{st_.mean(r[0] for r in ratios):.3f}, trips x{st_.mean(r[1] for r in ratios):.3f} "
      f"(mean trips {st_.mean(r[2] for r in ratios):.1f}, max trips {st_.mean(r[3] for r in ratios):.1f})")

# where did the slow waves of the last launch run, and what did they carry?
REC = 16  # words per wave record (brs_kernels.hip: brs_dbg_wave)
wb = (C.c_ulonglong * (REC * 1024))()
L.brs_debug_waves(wb)
import numpy as np
w = np.array(list(wb), dtype=np.uint64).reshape(1024, REC)
cyc, trips, hw, xcc = w[:, 8].astype(float), w[:, 9].astype(float), w[:, 12], w[:, 13] & 0xF
ph = w[:, :12].astype(float)
keys = np.stack([(w[:, 14] >> np.uint64(8 * k)) & np.uint64(0xFF) for k in range(8)], 1).astype(int)    # lanes per cost-class key
bucks = np.stack([(w[:, 15] >> np.uint64(8 * k)) & np.uint64(0xFF) for k in range(8)], 1).astype(int)   # lanes per bucket
print(f"  last launch: cycles/trip mean {np.mean(cyc / trips):.0f} min {np.min(cyc / trips):.0f} max {np.max(cyc / trips):.0f}; corr(cycles, trips) {np.corrcoef(cyc, trips)[0, 1]:.2f}")
for x in range(8):
    m = xcc == x
    if m.any(): print(f"    XCC {x}: waves {int(m.sum())} mean cycles {cyc[m].mean():.0f} max {cyc[m].max():.0f} cycles/trip {np.mean(cyc[m] / trips[m]):.0f}")


# cost-class key (brs_state.hpp: cost_class): bit 0 block can reach the floor, bit 1 a wheel, bit 2 NOT the torso
def kname(k):
    s = "+".join(n for b, n in ((1, "floor"), (2, "wheel")) if k & b) or "plain"
    return s + (" far" if k & 4 else "")


def row(label, m):
    c, t = cyc[m], trips[m]
    pt = lambda j: ph[m, j].sum() / t.sum()
    print(f"    {label:34s} {int(m.sum()):5d} {c.mean():10.0f} {c.max():10.0f} {t.mean():6.1f} {c.sum() / t.sum():7.0f} "
          f"{pt(2):6.0f} {pt(10):6.0f} {pt(11):6.0f} {pt(4):6.0f} {pt(5):6.0f}")


hdr = (f"    {'':34s} {'waves':>5s} {'mean cyc':>10s} {'max cyc':>10s} {'trips':>6s} {'cyc/trp':>7s} {'blkflr':>6s} {'patch':>6s} "
       f"{'wheels':>6s} {'assem':>6s} {'chol':>6s}   (phase columns: cycles per trip)")
print("  by composition (the set of cost-class keys present in the wave; far lanes only ride along):")
print(hdr)
comp = [tuple(k for k in range(8) if keys[i, k] and not (k == 4)) for i in range(1024)]
for cset in sorted(set(comp), key=lambda cs: -np.mean([cyc[i] for i in range(1024) if comp[i] == cs])):
    m = np.array([c == cset for c in comp])
    row(" | ".join(kname(k) for k in cset) or "far only", m)
print("  by key: waves holding >= 1 lane of it")
print(hdr)
for k in range(8):
    m = keys[:, k] > 0
    if m.any(): row(f"{k} {kname(k)} ({keys[:, k].sum()} lanes)", m)
print("  by bucket of the lane map (slot order): waves holding >= 1 lane of it")
print(hdr)
for b in range(8):
    m = bucks[:, b] > 0
    if m.any(): row(f"bucket {b} ({bucks[:, b].sum()} lanes)", m)
mixed = (bucks > 0).sum(1) > 1
print(f"  waves holding lanes of more than one bucket: {int(mixed.sum())}")
order = np.argsort(-cyc)[:16]
print("  slowest waves: wave cycles trips | lanes per key")
for i in order:
    print(f"    #{int(i):4d} {cyc[i]:10.0f} {trips[i]:4.0f} | " + ", ".join(f"{kname(k)} {keys[i, k]}" for k in range(8) if keys[i, k]))
if out_dir:  # the raw records (1024 waves x 16 words) for offline analysis
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, f"wave_records_{env}.npy"), w)
