"""Inputs and models shared by tests/test_qactor_cpu.py and tests/test_qactor_gpu.py (the int8 off-policy actor).
Model dicts are those of tests/ref_qactor.py."""
import copy

import numpy as np

from balance_robot_mujoco_rl_amd import _lib
from tests.qpolicy_cases import seeded_obs, special_rows  # noqa: F401

SIZES = ((6, 300), (300, 200), (200, 2))
NACTOR = 300 * 6 + 300 + 200 * 300 + 200 + 2 * 200 + 2
# the units at the edges of the 32-unit tiles and of the padding (300 -> 320, 200 -> 224)
EDGE_UNITS = ((0, 31, 32, 287, 288, 299), (0, 31, 32, 191, 192, 199))
# the best row of profiles/r01_pd_sweep_env03v2.json (tools/pd_sweep.py): kp, kd, kv, kyaw
PD_GAINS = (5.0, 2.0, -0.05, 0.05)


def random_model(seed, shift_ends_on_output=False):
    """weights uniform in [-127, 127], a NON-ZERO zero point on every tensor, the hidden out_zero included (step 4's general form
    and the fold), multipliers log-uniform over the range in which outputs neither all saturate nor all vanish, plus one channel
    per hidden layer (2 and 3) at each end of the valid shifts (t = 62 and t = 1).  `shift_ends_on_output`: the two output channels sit
    at those ends instead (their codes are then constant or saturated: a model for exactness, not for variety)"""
    rng = np.random.default_rng(1000 + seed)
    nz = lambda lo, hi: int(rng.choice([v for v in range(lo, hi + 1) if v != 0]))
    model = dict(input_scale=float(rng.uniform(0.03, 0.07)), input_zero=nz(-20, 20),
                 action_scale=float(rng.uniform(0.8, 1.2) / 128), action_zero=nz(-5, 5), layers=[])
    # |acc| is about sqrt(n_in) x 73 (rms weight) x the rms input: 2^13.5 behind 6 inputs, 2^17 behind 300 or 200 ReLU codes
    for k, (n_in, n_out) in enumerate(SIZES):
        lg = (rng.uniform(-8, -6), rng.uniform(-11.5, -10), rng.uniform(-11.5, -10))[k]
        M = 2.0 ** (lg + rng.uniform(-1, 1, n_out))
        if shift_ends_on_output and k == 2:
            M[0], M[1] = 2.0 ** -31.3, 2.0 ** 29.5
        elif k < 2:
            M[2], M[3] = 2.0 ** -31.3, 2.0 ** 29.5   # not on an edge unit: those must carry signal in edge_unit_model
        os_ = float(rng.uniform(0.01, 0.02))
        model["layers"].append(dict(W=rng.integers(-127, 128, (n_out, n_in)).astype(np.int64),
                                    b=rng.integers(-20000, 20001, n_out).astype(np.int64), bs=M * os_, os=os_,
                                    oz=nz(-100, -40) if k < 2 else nz(-30, 30)))
    return model


def edge_unit_model(layer, unit):
    """random_model(0) in which the layer after hidden layer `layer` reads ONLY `unit`, with weight +-127: the action code is then a
    known function of one accumulator, and an off-by-one at a tile or padding edge cannot hide behind 299 other terms"""
    model = copy.deepcopy(random_model(0))
    rng = np.random.default_rng(7 * unit + layer)
    L = model["layers"][layer + 1]
    n_out = L["W"].shape[0]
    L["W"][:] = 0
    L["W"][:, unit] = 127 * rng.choice([-1, 1], n_out)
    if n_out == 2:
        L["W"][:, unit] = (127, -127)
    # |acc| is at most 127 x 255: a multiplier near 2^-8 spreads it over the int8 range
    L["bs"] = 2.0 ** (-8 + rng.uniform(-0.5, 0.5, n_out)) * L["os"]
    L["b"] = rng.integers(-2000, 2001, n_out).astype(np.int64)
    return model


def pd_actor_params(seed=0):
    """A hand-built float actor [NACTOR]: the linear law of tools/pd_sweep.py, u = kp pitch + kd pitch' + kv (wl - wr) / 2 and
    yaw = kyaw (wl + wr), action = tanh((-u - yaw, u - yaw)), embedded exactly through ReLU pairs, relu(f) - relu(-f) = f, across
    both hidden layers (units 0..3 of each); the other units get small seeded weights so that all channels carry signal.  The
    deterministic, training-free stand-in for a trained actor."""
    kp, kd, kv, kyaw = PD_GAINS
    rng = np.random.default_rng(seed)
    u = np.array([0.25 * kp, kd, 0.5 * 42.5 * kv, -0.5 * 42.5 * kv, 0.0, 0.0])
    yaw = np.array([0.0, 0.0, 42.5 * kyaw, 42.5 * kyaw, 0.0, 0.0])
    W0, b0 = rng.normal(0, 0.05, (300, 6)), rng.normal(0, 0.05, 300)
    W0[:4], b0[:4] = (u, -u, yaw, -yaw), 0.0
    W1, b1 = rng.normal(0, 0.01, (200, 300)), rng.normal(0, 0.05, 200)
    W1[:4], b1[:4] = 0.0, 0.0
    W1[:, :4] = 0.0                      # the law's units feed only their own copies
    W1[np.arange(4), np.arange(4)] = 1.0
    W2, b2 = rng.normal(0, 0.002, (2, 200)), np.zeros(2)
    W2[:, :4] = ((-1, 1, -1, 1), (1, -1, -1, 1))
    flat = np.concatenate([W0.ravel(), b0, W1.ravel(), b1, W2.ravel(), b2]).astype(np.float32)
    assert flat.size == NACTOR
    return flat


def pd_law(obs):
    """the linear law itself, before the tanh: what pd_actor_params embeds (fp64)"""
    kp, kd, kv, kyaw = PD_GAINS
    o = np.asarray(obs, np.float64)
    u = kp * 0.25 * o[:, 0] + kd * o[:, 1] + kv * 42.5 * 0.5 * (o[:, 2] - o[:, 3])
    yaw = kyaw * 42.5 * (o[:, 2] + o[:, 3])
    return np.stack([-u - yaw, u - yaw], 1)


def sb3_init_params(seed=0):
    """an actor with the default initialisation of torch.nn.Linear, which SB3 keeps for TD3Policy: U(-1/sqrt(n_in), 1/sqrt(n_in))
    for weights and biases"""
    rng = np.random.default_rng(seed)
    parts = []
    for n_in, n_out in SIZES:
        bound = 1.0 / np.sqrt(n_in)
        parts += [rng.uniform(-bound, bound, n_out * n_in), rng.uniform(-bound, bound, n_out)]
    return np.concatenate(parts).astype(np.float32)


def in_box_obs(n, seed=1):
    """seeded observations inside the box REFERENCE_CALIBRATION spans"""
    return (np.random.default_rng(seed).uniform(-1, 1, (n, 6)) * [1.57, 6.28, 4, 4, 4, 4]).astype(np.float32)


def as_ref_model(qm):
    """the package's QuantActorModel -> a model dict"""
    return dict(input_scale=qm.input_scale, input_zero=qm.input_zero, action_scale=qm.action_scale, action_zero=qm.action_zero,
                layers=[{k: L[k] for k in ("W", "b", "bs", "os", "oz")} for L in qm.layers])


def all_models():
    """[(name, model dict)]: three random, the output layer at the shift ends, twelve edge units, the quantised PD actor"""
    from balance_robot_mujoco_rl_amd import quantize_actor
    return [(f"random/{s}", random_model(s)) for s in range(3)] + [("random/shift-ends-on-output", random_model(3, True))] + \
           [(f"edge/layer{k}/unit{u}", edge_unit_model(k, u)) for k in range(2) for u in EDGE_UNITS[k]] + \
           [("pd", as_ref_model(quantize_actor(pd_actor_params())))]


def c_model(model):
    """a model dict -> (include/brs_qpolicy.h brs_qactor_model, arrays to keep alive)"""
    from tests import ref_qactor as R
    m = _lib.BrsQActorModel()
    m.input_scale, m.input_zero = model["input_scale"], model["input_zero"]
    m.action_scale, m.action_zero = model["action_scale"], model["action_zero"]
    keep = []
    for k, L in enumerate(model["layers"]):
        W, b = np.ascontiguousarray(L["W"], np.int8), np.ascontiguousarray(L["b"], np.int32)
        bs = np.ascontiguousarray(L["bs"], np.float64)
        c = m.layer[k]
        c.n_out, c.n_in = W.shape
        c.weight, c.bias, c.bias_scale = W.ctypes.data, b.ctypes.data, bs.ctypes.data
        c.out_scale, c.out_zero, c.tanh_zero, c.tanh_table = L["os"], L["oz"], 0, None
        keep += [W, b, bs]
    t = np.ascontiguousarray(R.tanh_table(model), np.int8)
    m.layer[2].tanh_table = t.ctypes.data
    keep.append(t)
    return m, keep


def quant_model(model):
    """a model dict -> the package's QuantActorModel (weight scales are not part of the int8 arithmetic: set to bias scale / input
    scale, as the quantiser defines them)"""
    from balance_robot_mujoco_rl_amd.quant import QuantActorModel
    layers, in_scale = [], model["input_scale"]
    for L in model["layers"]:
        layers.append(dict(W=np.asarray(L["W"], np.int8), b=np.asarray(L["b"], np.int32), ws=np.asarray(L["bs"]) / in_scale, bs=L["bs"],
                           os=L["os"], oz=L["oz"]))
        in_scale = L["os"]
    return QuantActorModel(model["input_scale"], model["input_zero"], layers, model["action_scale"], model["action_zero"])
