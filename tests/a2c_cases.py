"""What the CPU and the GPU tests of the A2C learner share (tests/test_a2c_cpu.py, tests/test_a2c_gpu.py): the host build of the
kernel source behind DeviceA2CLearner's surface, the inputs with their condition (computed once per case) and the gate."""
import ctypes as C
import os
import subprocess

import numpy as np

import ref_a2c as A
import ref_learner as R
from balance_robot_mujoco_rl_amd import _lib
from learner_cases import GXX, N_ROWS, ROOT

HOST_DIR = os.path.join(ROOT, "tests", "a2chost")
NPARAM, NSTAT = R.NPARAM, R.NSTAT
MAX_DRAWS = 20


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class HostA2C:
    """tests/a2chost/a2chost.cpp with DeviceA2CLearner's surface, on numpy arrays"""

    def __init__(self, L, cfg, params, max_workgroups=0):
        self.L, self.cfg = L, cfg
        self.h = C.c_void_p(L.ah_create(max_workgroups))
        self.params = np.array(params, np.float32)
        self.sq = np.ones(NPARAM, np.float32)
        self.grad_buf = np.zeros(NPARAM + NSTAT, np.float32)

    def grad_rc(self, case, idx, m=None):
        idx = None if idx is None else np.ascontiguousarray(idx, np.int32)
        n = case["obs"].shape[0]
        cfg = self.cfg.c() if self.cfg is not None else None
        return self.L.ah_grad(self.h, _ptr(self.params), n, _ptr(case["obs"]), _ptr(case["act"]), _ptr(case["adv"]), _ptr(case["ret"]), _ptr(idx),
                              (n if idx is None else idx.size) if m is None else m, None if cfg is None else C.byref(cfg), _ptr(self.grad_buf))

    def grad(self, case, idx=None):
        rc = self.grad_rc(case, idx)
        assert rc == 0, rc
        return self.grad_buf.copy()

    def apply(self, grad=None):
        g = self.grad_buf if grad is None else np.ascontiguousarray(grad, np.float32)
        cfg = self.cfg.c()
        assert self.L.ah_apply(self.h, _ptr(self.params), _ptr(g), _ptr(self.sq), C.byref(cfg)) == 0

    def stats(self):
        s = _lib.BrsLearnerInfo()
        self.L.ah_stats(self.h, C.byref(s))
        return s

    def close(self):
        self.L.ah_destroy(self.h)


def build_host(directory):
    """g++ -> liba2chost.so in `directory`, with its signatures applied"""
    so = os.path.join(str(directory), "liba2chost.so")
    subprocess.check_call(GXX + ["-fPIC", "-shared", "-o", so, os.path.join(HOST_DIR, "a2chost.cpp")])
    L = C.CDLL(so)
    vp, cfg = C.c_void_p, C.POINTER(_lib.BrsA2cConfig)
    L.ah_create.restype, L.ah_create.argtypes = vp, [C.c_int]
    L.ah_destroy.restype, L.ah_destroy.argtypes = None, [vp]
    L.ah_grad.restype, L.ah_grad.argtypes = C.c_int, [vp, vp, C.c_int, vp, vp, vp, vp, vp, C.c_int, cfg, vp]
    L.ah_apply.restype, L.ah_apply.argtypes = C.c_int, [vp, vp, vp, vp, cfg]
    L.ah_stats.restype, L.ah_stats.argtypes = None, [vp, C.POINTER(_lib.BrsLearnerInfo)]
    L.ah_rmsprop.restype, L.ah_rmsprop.argtypes = None, [vp, vp, vp, C.c_int, cfg]
    return L


_ROLLOUTS, _CASES = {}, {}


def _rollout(seed):
    """ref_learner.make_case's rollout of N_ROWS rows (its logp_old is ignored: A2C has none); drawn once per seed, never changed"""
    if seed not in _ROLLOUTS:
        _ROLLOUTS[seed] = R.make_case(N_ROWS, seed)
    return _ROLLOUTS[seed]


def head(case, m):
    """the first m rows as a rollout of its own: what idx = None walks"""
    return {**case, **{k: np.ascontiguousarray(case[k][:m]) for k in A.KEYS}}


# the first seed whose draw passes the condition, where seed 0's does not (found with tests/ref_a2c.py::kappa on the CPU)
SEEDS = {64: 2, 65: 1, 255: 3}


def conditioned(m, cfg=A.Cfg(), seed=None, whole=False):
    """-> (case, idx): a rollout and m of its rows (drawn with repeats; `whole`: the rollout is cut to its first m rows and idx is
    None) that pass the input condition for `cfg`, kappa <= 4 on the sums behind pi.b3 and vf.b3 in fp64.  A draw that violates it
    is drawn again with the next seed; no draw among MAX_DRAWS fails the test.  The seeds the tests pass were picked with the
    reference alone, so that every case passes on its first or second draw"""
    if seed is None:
        seed = 0 if whole else SEEDS.get(m, 0)
    key = (m, seed, whole, cfg.normalize_adv, cfg.ent_coef, cfg.actor_on, cfg.ret_scale, cfg.vf_coef)
    if key not in _CASES:
        for draw in range(MAX_DRAWS):
            case = _rollout(seed + draw)
            if whole:
                case, idx = head(case, m), None
            else:
                idx = R.make_idx(N_ROWS, m)
                if m > 2:
                    idx[1] = idx[0]   # a repeated index, whatever the draw
            k = A.kappa(case, idx, cfg)
            if k <= A.KAPPA_MAX:
                _CASES[key] = (case, idx)
                break
        else:
            raise AssertionError(f"m={m} seed={seed}: no draw among {MAX_DRAWS} satisfies kappa <= {A.KAPPA_MAX}")
    return _CASES[key]


def gate(g, g64, what):
    err = R.block_errors(g, g64)
    worst = max(err, key=err.get)
    print(f"{what}: largest |g - g64| / |g64| per block = {err[worst]:.3g} ({worst})")
    assert err[worst] <= R.GATE, err
    R.stats_close(g, g64)
    assert g[NPARAM + 3] == 0.0 and g[NPARAM + 4] == 0.0   # the KL and clip-fraction slots
