"""Independent restatement of the int8 off-policy actor of include/brs_qpolicy.h (6 -> 300 -> ReLU -> 200 -> ReLU -> 2 -> tanh,
steps 1-6): numpy only, no code from the package; the multiplier decomposition is tests/ref_qpolicy.py's.  Test
infrastructure: the kernel and its host build are compared with this, exactly.

A model is a dict: input_scale, input_zero, action_scale, action_zero, layers = three dicts with W int [out][in], b int [out],
bs float64 [out] (bias scale), os, oz (output scale / zero point).  Only the output layer has a table (tanh_table)."""
import numpy as np

from tests.ref_qpolicy import multiplier

I32_MAX = 2 ** 31 - 1


def tanh_table(model):
    """step 5's table, indexed by q + 128 (fp64, half to even)"""
    L = model["layers"][2]
    j = np.arange(256, dtype=np.float64)
    return np.clip(np.rint(np.tanh((j - 128 - L["oz"]) * L["os"]) / model["action_scale"]) + model["action_zero"], -128, 127).astype(np.int64)


def act(model, obs, hidden=False):
    """obs [n, 6] float32 -> (action [n, 2] float32, codes [n, 2] int8); hidden=True: also the two hidden layers' codes"""
    x = np.asarray(obs, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        v = np.rint(x / np.float64(model["input_scale"]))                     # 1. IEEE fp64 division, half to even
    v = np.where(np.isnan(v), 0.0, v) + model["input_zero"]                   #    NaN -> the zero point
    q = np.clip(v, -128.0, 127.0).astype(np.int64)                            #    clamp, then to integer
    z, codes = model["input_zero"], []
    for k, L in enumerate(model["layers"]):
        W, b = np.asarray(L["W"], np.int64), np.asarray(L["b"], np.int64)
        # 2.  The integer product as an fp64 one: |q - z| <= 255, |W| <= 128, at most 300 terms, so every partial sum is an
        #     integer below 2^24 and fp64 (exact to 2^53) holds it exactly in any order of summation
        acc = b + ((q - z).astype(np.float64) @ W.T.astype(np.float64)).astype(np.int64)
        assert np.abs(acc).max() <= I32_MAX
        mt = [multiplier(float(bs) / L["os"]) for bs in np.asarray(L["bs"], np.float64)]
        m, t = np.array([a[0] for a in mt], np.int64), np.array([a[1] for a in mt], np.int64)
        q = np.clip(((acc * m + np.left_shift(np.int64(1), t - 1)) >> t) + L["oz"], -128, 127)   # 3. one rounding
        if k < 2:
            q, z = np.maximum(q, L["oz"]), L["oz"]                            # 4. ReLU: the code of real 0 is the floor
            codes.append(q)
    q = tanh_table(model)[q + 128]                                            # 5.
    a = ((q - model["action_zero"]).astype(np.float64) * np.float64(model["action_scale"])).astype(np.float32)   # 6.
    return (a, q.astype(np.int8), codes) if hidden else (a, q.astype(np.int8))


def float_actor(flat, obs):
    """the float network in fp64: flat DDPG actor vector [62702], obs [n, 6] -> action [n, 2]"""
    flat, x, off = np.asarray(flat, np.float64), np.asarray(obs, np.float64), 0
    for k, (n_in, n_out) in enumerate(((6, 300), (300, 200), (200, 2))):
        W = flat[off:off + n_in * n_out].reshape(n_out, n_in); off += n_in * n_out
        b = flat[off:off + n_out]; off += n_out
        x = x @ W.T + b
        x = np.maximum(x, 0.0) if k < 2 else np.tanh(x)
    return x
