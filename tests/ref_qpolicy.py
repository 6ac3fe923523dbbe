"""Independent restatement of the int8 actor of include/brs_qpolicy.h (steps 1-5): numpy int64 only, math.frexp for the
multiplier, no code from the package.  Test infrastructure: the kernel, its host build and the existing evaluator
(tests/quant_policy.py) are all compared with this, exactly.

A model is a dict: input_scale, input_zero, layers = three dicts with W int [out][in], b int [out], bs float64 [out]
(bias scale), os, oz (output scale / zero point) and, on the two hidden layers, ts, tz (scale / zero point of the tanh)."""
import math

import numpy as np

I32_MAX = 2 ** 31 - 1


def multiplier(M):
    """M = m 2^-t with m in [2^30, 2^31): (m, t), or None where brs_qpolicy_quantize_multiplier returns BRS_ERR_ARG"""
    if not (M > 0.0) or math.isinf(M) or math.isnan(M):
        return None
    f, e = math.frexp(M)
    m = int(math.floor(f * 2.0 ** 31 + 0.5))
    if m == 2 ** 31:
        m, e = 2 ** 30, e + 1
    t = 31 - e
    return (m, t) if 1 <= t <= 62 else None


def tanh_table(L):
    """step 4's table for hidden layer L, indexed by q + 128"""
    j = np.arange(256, dtype=np.float64)
    return np.clip(np.rint(np.tanh((j - 128 - L["oz"]) * L["os"]) / L["ts"]) + L["tz"], -128, 127).astype(np.int64)


def from_npz(path, head="actions"):
    """the key set of tests/golden/robot_move_policy.npz"""
    z = np.load(path)
    s = lambda k: float(np.asarray(z[k], np.float64).ravel()[0])
    layers = []
    for k in range(3):
        pre = "fc2_mean" if (k == 2 and head == "mean") else f"fc{k}"
        L = dict(W=np.asarray(z[f"fc{k}_weight_q"], np.int64), b=np.asarray(z[f"{pre}_bias_q"], np.int64),
                 bs=np.asarray(z[f"{pre}_bias_scale"], np.float64), os=s(f"{pre}_out_scale"), oz=int(s(f"{pre}_out_zero_point")))
        if k < 2:
            L["ts"], L["tz"] = s(f"tanh{k}_out_scale"), int(s(f"tanh{k}_out_zero_point"))
        layers.append(L)
    return dict(input_scale=s("input_scale"), input_zero=int(s("input_zero_point")), layers=layers)


def act(model, obs):
    """obs [n, 6] float32 -> (action [n, 2] float32, codes [n, 2] int8)"""
    x = np.asarray(obs, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        v = np.rint(x / np.float64(model["input_scale"]))                     # 1. IEEE fp64 division, half to even
    v = np.where(np.isnan(v), 0.0, v) + model["input_zero"]                   #    NaN -> the zero point
    q = np.clip(v, -128.0, 127.0).astype(np.int64)                            #    clamp, then to integer
    z = model["input_zero"]
    for k, L in enumerate(model["layers"]):
        W, b = np.asarray(L["W"], np.int64), np.asarray(L["b"], np.int64)
        acc = b + (q - z) @ W.T                                               # 2.
        assert np.abs(acc).max() <= I32_MAX
        mt = [multiplier(float(bs) / L["os"]) for bs in np.asarray(L["bs"], np.float64)]
        m, t = np.array([a[0] for a in mt], np.int64), np.array([a[1] for a in mt], np.int64)
        q = np.clip(((acc * m + np.left_shift(np.int64(1), t - 1)) >> t) + L["oz"], -128, 127)   # 3. one rounding
        if k < 2:
            q, z = tanh_table(L)[q + 128], L["tz"]                            # 4.
    return ((q - L["oz"]).astype(np.float64) * np.float64(L["os"])).astype(np.float32), q.astype(np.int8)   # 5.
