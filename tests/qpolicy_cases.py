"""Inputs and models shared by tests/test_qpolicy_cpu.py and tests/test_qpolicy_gpu.py (the int8 actor)."""
import os

import numpy as np

from balance_robot_mujoco_rl_amd import _lib

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "robot_move_policy.npz")


def seeded_obs(n):
    """in-range observations; every fourth row is scaled by 3 and saturates the input"""
    obs = (np.random.default_rng(0).uniform(-1, 1, (n, 6)) * [1.6, 6.3, 4, 4, 4, 4]).astype(np.float32)
    obs[::4] *= 3
    return obs


def special_rows():
    """rows of NaN, +-Inf, +-1e30, and in-range rows with one special value each"""
    vals = [np.nan, np.inf, -np.inf, 1e30, -1e30]
    rows = [np.full(6, v, np.float32) for v in vals]
    base = seeded_obs(8)[1]
    for k, v in enumerate(vals * 2):
        r = base.copy()
        r[k % 6] = v
        rows.append(r)
    return np.stack(rows).astype(np.float32)


def random_model(seed):
    """weights uniform in [-127, 127], a NON-ZERO zero point on every tensor (the fixture's hidden zero points are all 0,
    which would hide a wrong zero-point fold), multipliers log-uniform over the range in which outputs neither all
    saturate nor all vanish, plus one channel per layer at each end of the valid shifts (t = 62 and t = 1)"""
    rng = np.random.default_rng(seed)
    nz = lambda lo, hi: int(rng.choice([v for v in range(lo, hi + 1) if v != 0]))
    model = dict(input_scale=float(rng.uniform(0.03, 0.07)), input_zero=nz(-20, 20), layers=[])
    for k, (n_in, n_out) in enumerate(((6, 64), (64, 64), (64, 2))):
        lg = rng.uniform(-12, -8) if k else rng.uniform(-8, -5)
        M = 2.0 ** (lg + rng.uniform(-1, 1, n_out))
        if k < 2:
            M[0], M[1] = 2.0 ** -31.3, 2.0 ** 29.5
        os_ = float(rng.uniform(0.01, 0.05))
        L = dict(W=rng.integers(-127, 128, (n_out, n_in)).astype(np.int64), b=rng.integers(-20000, 20001, n_out).astype(np.int64),
                 bs=M * os_, os=os_, oz=nz(-30, 30))
        if k < 2:
            L["ts"], L["tz"] = float(rng.uniform(0.8, 1.2) / 128), nz(-5, 5)
        model["layers"].append(L)
    return model


def c_model(model, table=None):
    """a model dict of tests/ref_qpolicy.py -> (include/brs_qpolicy.h brs_qmodel, arrays to keep alive).  `table(k, L)`
    overrides the table pointer of hidden layer k (tests of the argument checks)"""
    from tests import ref_qpolicy as R
    m = _lib.BrsQModel()
    m.input_scale, m.input_zero, m.reserved = model["input_scale"], model["input_zero"], 0
    keep = []
    for k, L in enumerate(model["layers"]):
        W, b = np.ascontiguousarray(L["W"], np.int8), np.ascontiguousarray(L["b"], np.int32)
        bs = np.ascontiguousarray(L["bs"], np.float64)
        c = m.layer[k]
        c.n_out, c.n_in = W.shape
        c.weight, c.bias, c.bias_scale = W.ctypes.data, b.ctypes.data, bs.ctypes.data
        c.out_scale, c.out_zero = L["os"], L["oz"]
        keep += [W, b, bs]
        if k < 2:
            t = np.ascontiguousarray(R.tanh_table(L), np.int8)
            c.tanh_zero, c.tanh_table = L["tz"], t.ctypes.data
            keep.append(t)
    return m, keep


def quant_model(model):
    """a model dict -> the package's QuantModel (weight scales are not part of the int8 arithmetic: set to bias scale / input
    scale, as the quantiser defines them)"""
    from balance_robot_mujoco_rl_amd.quant import QuantModel
    layers, in_scale = [], model["input_scale"]
    for k, L in enumerate(model["layers"]):
        d = dict(W=np.asarray(L["W"], np.int8), b=np.asarray(L["b"], np.int32), ws=np.asarray(L["bs"]) / in_scale, bs=L["bs"], os=L["os"], oz=L["oz"])
        if k < 2:
            d["ts"], d["tz"] = L["ts"], L["tz"]
            in_scale = L["ts"]
        layers.append(d)
    return QuantModel(model["input_scale"], model["input_zero"], layers)
