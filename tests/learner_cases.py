"""What the CPU and the GPU tests of the PPO learner share (tests/test_learner_cpu.py, tests/test_learner_gpu.py): the host build
of the kernel source behind DevicePPOLearner's surface, the conditioned inputs (computed once per size) and the gate."""
import ctypes as C
import os
import subprocess

import numpy as np

import ref_learner as R
from balance_robot_mujoco_rl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_DIR = os.path.join(ROOT, "tests", "learnerhost")
GXX = ["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "balance_robot_mujoco_rl_amd", "csrc")]
N_ROWS = 3000
NPARAM, NSTAT = R.NPARAM, R.NSTAT


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class HostLearner:
    """tests/learnerhost/learnerhost.cpp with DevicePPOLearner's surface, on numpy arrays"""

    def __init__(self, L, cfg, params, max_workgroups=0):
        self.L, self.cfg = L, cfg
        self.h = C.c_void_p(L.lh_create(max_workgroups))
        self.params = np.array(params, np.float32)
        self.m, self.v = np.zeros(NPARAM, np.float32), np.zeros(NPARAM, np.float32)
        self.grad_buf = np.zeros(NPARAM + NSTAT, np.float32)

    def grad(self, case, idx):
        idx = np.ascontiguousarray(idx, np.int32)
        cfg = self.cfg.c()
        rc = self.L.lh_grad(self.h, _ptr(self.params), case["obs"].shape[0], _ptr(case["obs"]), _ptr(case["act"]), _ptr(case["logp_old"]),
                            _ptr(case["adv"]), _ptr(case["ret"]), _ptr(idx), idx.size, C.byref(cfg), _ptr(self.grad_buf))
        assert rc == 0, rc
        return self.grad_buf.copy()

    def apply(self, grad=None):
        g = self.grad_buf if grad is None else np.ascontiguousarray(grad, np.float32)
        cfg = self.cfg.c()
        assert self.L.lh_apply(self.h, _ptr(self.params), _ptr(g), _ptr(self.m), _ptr(self.v), C.byref(cfg)) == 0

    def begin_iteration(self):
        self.L.lh_begin_iteration(self.h)

    def stats(self):
        s = _lib.BrsLearnerInfo()
        self.L.lh_stats(self.h, C.byref(s))
        return s

    def close(self):
        self.L.lh_destroy(self.h)


def build_host(directory):
    """g++ -> liblearnerhost.so in `directory`, with its signatures applied"""
    so = os.path.join(str(directory), "liblearnerhost.so")
    subprocess.check_call(GXX + ["-fPIC", "-shared", "-o", so, os.path.join(HOST_DIR, "learnerhost.cpp")])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.lh_create.restype, L.lh_create.argtypes = vp, [C.c_int]
    L.lh_destroy.restype, L.lh_destroy.argtypes = None, [vp]
    L.lh_begin_iteration.restype, L.lh_begin_iteration.argtypes = None, [vp]
    L.lh_grad.restype, L.lh_grad.argtypes = C.c_int, [vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, C.POINTER(_lib.BrsPpoConfig), vp]
    L.lh_apply.restype, L.lh_apply.argtypes = C.c_int, [vp, vp, vp, vp, vp, C.POINTER(_lib.BrsPpoConfig)]
    L.lh_stats.restype, L.lh_stats.argtypes = None, [vp, C.POINTER(_lib.BrsLearnerInfo)]
    return L


_CASES = {}


def conditioned(m, cfg=R.Cfg(), seed=0):
    """the shared rollout (N_ROWS rows, seed 0) and an index list of m rows with repeats, conditioned for `cfg`; computed once"""
    key = (m, seed, cfg.clip_range, cfg.normalize_adv)
    if key not in _CASES:
        case, idx = R.make_case(N_ROWS, seed), R.make_idx(N_ROWS, m)
        if m > 2:
            idx[1] = idx[0]   # a repeated index, whatever the draw
        _CASES[key] = (R.condition(case, idx, cfg), idx)
    return _CASES[key]


def gate(g, g64, what):
    err = R.block_errors(g, g64)
    worst = max(err, key=err.get)
    print(f"{what}: largest |g - g64| / |g64| per block = {err[worst]:.3g} ({worst})")
    assert err[worst] <= R.GATE, err
    R.stats_close(g, g64)
