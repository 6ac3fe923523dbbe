"""int8 policies on the device (include/brs_qpolicy.h): the deployment check at the end of the reference's
pipeline.  The reference quantises a trained policy to int8 with the TFLite converter (src/quantize_tflite.py), then drives
the int8 network in closed loop in the simulator (src/sb_rl.py:285-364, `test-tflite-quant`) before it is flashed.

    QuantModel        the integer tensors, scales and zero points of an int8 actor; reads and writes the npz key set of
                      tests/golden/robot_move_policy.npz
    quantize_policy   post-training quantisation of the actor tower of a float parameter vector (DevicePolicy's) or an SB3
                      state_dict: no TFLite needed
    QuantPolicy       the int8 network for n envs as a HIP kernel (brs_qpolicy_act), bit-exact integer arithmetic
    QuantActorModel, quantize_actor, QuantActor
                      the same three for the off-policy actor 6 -> 300 -> ReLU -> 200 -> ReLU -> 2 -> tanh of DDPG, TD3 and SAC
                      (brs_qpolicy_actor_act), and for SAC's actor at SB3's default widths, 6 -> 256 -> 256 -> 2
                      (net_arch="sb3")

PyTorch only owns the buffers and the stream.  There is no CPU fallback."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._handle import Handle, _need, _p
from .nets import ARCH_NAMES, ARCHS
from .policy import NPARAM, flatten_sb3_state_dict

REFERENCE_CALIBRATION = np.array([[-3.14 / 2, -6.28, -4.0, -4.0, -4.0, -4.0],
                                  [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                                  [3.14 / 2, 6.28, 4.0, 4.0, 4.0, 4.0]], dtype=np.float64)
"""The representative dataset of the reference's converter script (src/quantize_tflite.py:9-13), as data: the two corners
of the observation box it expects, and the origin.  Default calibration of `quantize_policy`."""

_SIZES = ((6, 64), (64, 64), (64, 2))
_NPI = 64 * 6 + 64 + 64 * 64 + 64 + 2 * 64 + 2


def _round_half_away(x):
    x = np.asarray(x, np.float64)
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def _activation_qparams(lo, hi):
    """(scale, zero point) of an int8 activation whose range [lo, hi] is widened to include 0"""
    lo, hi = min(float(lo), 0.0), max(float(hi), 0.0)
    if not hi > lo:
        return 1.0, 0  # degenerate range: every value is 0
    scale = (hi - lo) / 255.0
    return scale, int(np.clip(_round_half_away(-128.0 - lo / scale), -128, 127))


def tanh_table(in_scale, in_zero, out_scale, out_zero):
    """the 256-entry table of a quantised tanh, indexed by q + 128 (fp64, half to even)"""
    q = np.arange(-128, 128, dtype=np.float64)
    return np.clip(np.rint(np.tanh((q - in_zero) * in_scale) / out_scale) + out_zero, -128, 127).astype(np.int8)


class QuantModel:
    """An int8 actor 6 -> 64 -> tanh -> 64 -> tanh -> 2.  `layers[k]` is a dict: W int8 [out][in], b int32 [out], ws float64
    [out] (weight scale per output channel), bs float64 [out] (bias scale = input scale x ws), os / oz (scale and zero point
    of the layer's output), and for the hidden layers ts / tz (scale and zero point of the tanh's output)."""

    def __init__(self, input_scale, input_zero, layers, value_tower=None):
        self.input_scale, self.input_zero = float(input_scale), int(input_zero)
        self.layers = []
        for k, (L, (n_in, n_out)) in enumerate(zip(layers, _SIZES)):
            W, b = np.asarray(L["W"]), np.asarray(L["b"])
            if W.shape != (n_out, n_in) or b.shape != (n_out,):
                raise ValueError(f"layer {k}: expected weights {(n_out, n_in)} and bias {(n_out,)}, got {W.shape} and {b.shape}")
            if np.abs(W).max(initial=0) > 128 or np.abs(b.astype(np.int64)).max(initial=0) > 2 ** 31 - 1:
                raise ValueError(f"layer {k}: weights must fit int8 and biases int32")
            d = dict(W=np.ascontiguousarray(W, np.int8), b=np.ascontiguousarray(b, np.int32),
                     ws=np.ascontiguousarray(np.broadcast_to(np.asarray(L["ws"], np.float64).ravel(), (n_out,))),
                     bs=np.ascontiguousarray(np.broadcast_to(np.asarray(L["bs"], np.float64).ravel(), (n_out,))),
                     os=float(L["os"]), oz=int(L["oz"]))
            if k < 2:
                d["ts"], d["tz"] = float(L["ts"]), int(L["tz"])
            self.layers.append(d)
        self.value_tower = value_tower  # {npz key: array} of the vf* keys, or None

    # ------------------------------------------------------------------------------------------------------------ files
    @classmethod
    def load(cls, path, head="actions"):
        """read the npz key set of tests/golden/robot_move_policy.npz.  head = "actions": the tensor the reference reads
        (fc2_*); "mean": the distribution mean of the same export (fc2_mean_* for the bias and the output)"""
        if head not in ("actions", "mean"):
            raise ValueError(f"head must be 'actions' or 'mean', got {head!r}")
        z = np.load(path)  # allow_pickle stays False
        s = lambda k: float(np.asarray(z[k], np.float64).ravel()[0])
        layers = []
        for k in range(3):
            pre = "fc2_mean" if (k == 2 and head == "mean") else f"fc{k}"
            L = dict(W=z[f"fc{k}_weight_q"], ws=z[f"fc{k}_weight_scale"], b=z[f"{pre}_bias_q"], bs=z[f"{pre}_bias_scale"],
                     os=s(f"{pre}_out_scale"), oz=int(s(f"{pre}_out_zero_point")))
            if k < 2:
                L["ts"], L["tz"] = s(f"tanh{k}_out_scale"), int(s(f"tanh{k}_out_zero_point"))
            layers.append(L)
        vf = {k: np.asarray(z[k]) for k in z.files if k.startswith("vf")}
        return cls(s("input_scale"), int(s("input_zero_point")), layers, vf or None)

    def arrays(self):
        """the npz key set, fc2_mean_* equal to fc2_*"""
        i64 = lambda v, n=1: np.full(n, int(v), np.int64)
        out = {"input_scale": np.array([self.input_scale]), "input_zero_point": i64(self.input_zero)}
        for k, L in enumerate(self.layers):
            n_out = L["W"].shape[0]
            for pre in ([f"fc{k}"] if k < 2 else ["fc2", "fc2_mean"]):
                if pre != "fc2_mean":
                    out[f"{pre}_weight_q"], out[f"{pre}_weight_scale"], out[f"{pre}_weight_zero_point"] = L["W"], L["ws"], i64(0, n_out)
                out[f"{pre}_bias_q"], out[f"{pre}_bias_scale"], out[f"{pre}_bias_zero_point"] = L["b"], L["bs"], i64(0, n_out)
                out[f"{pre}_out_scale"], out[f"{pre}_out_zero_point"] = np.array([L["os"]]), i64(L["oz"])
            if k < 2:
                out[f"tanh{k}_out_scale"], out[f"tanh{k}_out_zero_point"] = np.array([L["ts"]]), i64(L["tz"])
        out.update(self.value_tower or {})
        return out

    def save(self, path):
        np.savez(path, **self.arrays())

    # --------------------------------------------------------------------------------------------------------- contents
    def float_params(self):
        """the same network with DEQUANTISED weights as the flat float32 vector of include/brs_policy.h (what
        DevicePolicy.set_weights takes); the value tower is zeros when the file had none, log_std = 0"""
        parts = []
        for L in self.layers:
            parts += [(L["W"].astype(np.float64) * L["ws"][:, None]).ravel(), L["b"].astype(np.float64) * L["bs"]]
        vf = self.value_tower
        for k, (n_in, n_out) in enumerate(((6, 64), (64, 64), (64, 1))):
            if vf and f"vf{k}_weight_q" in vf:
                ws = np.asarray(vf[f"vf{k}_weight_scale"], np.float64).ravel()
                parts += [(np.asarray(vf[f"vf{k}_weight_q"], np.float64) * (ws[:, None] if ws.size == n_out else ws)).ravel(),
                          np.asarray(vf[f"vf{k}_bias_q"], np.float64) * np.asarray(vf[f"vf{k}_bias_scale"], np.float64)]
            else:
                parts += [np.zeros(n_in * n_out), np.zeros(n_out)]
        flat = np.concatenate(parts + [np.zeros(2)]).astype(np.float32)
        assert flat.size == NPARAM
        return flat

    def tables(self):
        """the tanh tables of the two hidden layers, int8 [2][256], indexed by q + 128"""
        return np.stack([tanh_table(L["os"], L["oz"], L["ts"], L["tz"]) for L in self.layers[:2]])

    def c_model(self):
        """-> (include/brs_qpolicy.h brs_qmodel, the arrays its pointers refer to: keep them alive while it is used)"""
        m = _lib.BrsQModel()
        m.input_scale, m.input_zero, m.reserved = self.input_scale, self.input_zero, 0
        tables = self.tables()
        keep = [tables]
        for k, L in enumerate(self.layers):
            c = m.layer[k]
            c.n_in, c.n_out = L["W"].shape[1], L["W"].shape[0]
            c.weight, c.bias, c.bias_scale = L["W"].ctypes.data, L["b"].ctypes.data, L["bs"].ctypes.data
            c.out_scale, c.out_zero = L["os"], L["oz"]
            c.tanh_zero = L["tz"] if k < 2 else 0
            c.tanh_table = tables[k].ctypes.data if k < 2 else None
            keep += [L["W"], L["b"], L["bs"]]
        return m, keep


def quantize_policy(params, calibration_obs=None):
    """Post-training int8 quantisation of the ACTOR tower of a float policy -> QuantModel.  `params`: the flat parameter
    vector of include/brs_policy.h (DevicePolicy / DeviceRollout) or an SB3 MlpPolicy state_dict; `calibration_obs` [k, 6]:
    observations that span the ranges the robot will see (default: REFERENCE_CALIBRATION).

    Every rounding is half away from zero.  An activation's range always includes 0: scale = (hi - lo) / 255, zero point =
    clamp(round(-128 - lo / scale)); a degenerate range gets scale 1.  Weights are symmetric per output channel: ws =
    max|row| / 127 (1 for an all-zero row), codes clipped to +-127.  bias_scale = input scale x ws, bias_q = round(b /
    bias_scale).  The ranges of the pre-activations are those of the FLOAT network, evaluated in fp64 on the calibration
    rows.  Every tanh output has scale 1 / 128 and zero point 0."""
    flat = flatten_sb3_state_dict(params) if isinstance(params, dict) else np.asarray(params)
    if flat.size != NPARAM:
        raise ValueError(f"expected {NPARAM} parameters, got {flat.size}")
    flat = flat.astype(np.float64).ravel()
    cal = np.asarray(REFERENCE_CALIBRATION if calibration_obs is None else calibration_obs, np.float64)
    if cal.ndim != 2 or cal.shape[1] != 6 or cal.shape[0] < 1 or not np.isfinite(cal).all():
        raise ValueError("calibration_obs: expected finite [k, 6]")
    if not np.isfinite(flat[:_NPI]).all():
        raise ValueError("the actor's parameters are not finite")
    in_scale, in_zero = _activation_qparams(cal.min(), cal.max())
    input_scale, input_zero = in_scale, in_zero
    x, off, layers = cal, 0, []
    for k, (n_in, n_out) in enumerate(_SIZES):
        W = flat[off:off + n_in * n_out].reshape(n_out, n_in); off += n_in * n_out
        b = flat[off:off + n_out]; off += n_out
        amax = np.abs(W).max(axis=1)
        ws = np.where(amax > 0, amax / 127.0, 1.0)
        Wq = np.clip(_round_half_away(W / ws[:, None]), -127, 127).astype(np.int8)
        bs = in_scale * ws
        bq = _round_half_away(b / bs)
        if np.abs(bq).max() > 2 ** 31 - 1:
            raise ValueError(f"layer {k}: a quantised bias leaves int32 (bias {np.abs(b).max():.3g} at scale {bs.min():.3g})")
        pre = x @ W.T + b  # the float network on the calibration rows
        os_, oz = _activation_qparams(pre.min(), pre.max())
        L = dict(W=Wq, b=bq.astype(np.int32), ws=ws, bs=bs, os=os_, oz=oz)
        if k < 2:
            L["ts"], L["tz"] = 1.0 / 128.0, 0
            x, in_scale = np.tanh(pre), 1.0 / 128.0
        layers.append(L)
    return QuantModel(input_scale, input_zero, layers)


class QuantPolicy(Handle):
    """The int8 actor evaluated by the HIP kernel: obs [n, 6] -> action [n, 2], with integer arithmetic only"""
    _FAMILY, _WHAT = "brs_qpolicy", "the int8 policy has"

    def __init__(self, model, device=0):
        self._attach(device)
        self._create("brs_qpolicy_create", self.device.index)
        self.set_model(model)

    def set_model(self, model):
        """load another QuantModel (synchronous; takes effect on the next act)"""
        m, keep = model.c_model()
        self._check(self.L.brs_qpolicy_set_model(self.h, C.byref(m)), "brs_qpolicy_set_model")
        del keep
        self.model = model

    def act(self, obs, out=None, out_q=None):
        """obs [n, 6] f32 cuda -> action [n, 2] f32 (not clipped); `out_q` [n, 2] int8 receives the int8 codes"""
        n = obs.shape[0]
        d = self.device
        _need(obs, "obs", torch.float32, (n, 6), d)
        if out is None:
            out = torch.empty((n, 2), dtype=torch.float32, device=d)
        _need(out, "out", torch.float32, (n, 2), d)
        if out_q is not None:
            _need(out_q, "out_q", torch.int8, (n, 2), d)
        self._check(self.L.brs_qpolicy_act(self.h, n, _p(obs), _p(out), _p(out_q), self._stream()), "brs_qpolicy_act")
        return out


# ------------------------------------------------------------------- the off-policy actor, 6 -> 300 -> ReLU -> 200 -> ReLU -> 2 -> tanh
def _actor_sizes(net_arch):
    """(in, out) of the three layers the int8 actor kernel of `net_arch` is built for (nets.py's table)"""
    return ARCHS[net_arch].actor.sizes


class QuantActorModel:
    """An int8 actor 6 -> 300 -> ReLU -> 200 -> ReLU -> 2 -> tanh, the network DDPG, TD3 and SAC train, or
    6 -> 256 -> ReLU -> 256 -> ReLU -> 2 -> tanh, SAC's at SB3's default widths: the widths are read off the tensors, and
    `net_arch` says which they are ("reference" or "sb3").
    `layers[k]` is a dict: W int8 [out][in], b int32 [out], ws float64 [out] (weight scale per output channel), bs float64 [out]
    (bias scale = input scale x ws), os / oz (scale and zero point of the layer's output; on a hidden layer oz is the code of
    real 0, below which ReLU clamps).  `action_scale` / `action_zero`: of the output tanh table's result."""

    def __init__(self, input_scale, input_zero, layers, action_scale=1.0 / 128.0, action_zero=0):
        self.input_scale, self.input_zero = float(input_scale), int(input_zero)
        self.action_scale, self.action_zero = float(action_scale), int(action_zero)
        if len(layers) != 3:
            raise ValueError(f"expected three layers, got {len(layers)}")
        self.layers = []
        shape0 = np.asarray(layers[0]["W"]).shape
        self.net_arch = next((name for name, arch in ARCHS.items() if shape0 == arch.actor.shapes[0][0]), None)
        if self.net_arch is None:
            raise ValueError(f"layer 0: expected weights (300, 6) (net_arch 'reference') or (256, 6) ('sb3'), got {shape0}")
        other = "sb3" if self.net_arch == "reference" else "reference"
        for k, (L, (n_in, n_out), (o_in, o_out)) in enumerate(zip(layers, _actor_sizes(self.net_arch), _actor_sizes(other))):
            W, b = np.asarray(L["W"]), np.asarray(L["b"])
            if W.shape != (n_out, n_in) or b.shape != (n_out,):
                raise ValueError(f"layer {k}: expected weights {(n_out, n_in)} and bias {(n_out,)} (net_arch {self.net_arch!r}; {other!r} has "
                                 f"{(o_out, o_in)} and {(o_out,)}), got {W.shape} and {b.shape}")
            if np.abs(W).max(initial=0) > 128 or np.abs(b.astype(np.int64)).max(initial=0) > 2 ** 31 - 1:
                raise ValueError(f"layer {k}: weights must fit int8 and biases int32")
            self.layers.append(dict(W=np.ascontiguousarray(W, np.int8), b=np.ascontiguousarray(b, np.int32),
                                    ws=np.ascontiguousarray(np.broadcast_to(np.asarray(L["ws"], np.float64).ravel(), (n_out,))),
                                    bs=np.ascontiguousarray(np.broadcast_to(np.asarray(L["bs"], np.float64).ravel(), (n_out,))),
                                    os=float(L["os"]), oz=int(L["oz"])))

    # ------------------------------------------------------------------------------------------------------------ files
    @classmethod
    def load(cls, path):
        z = np.load(path)  # allow_pickle stays False
        s = lambda k: float(np.asarray(z[k], np.float64).ravel()[0])
        layers = [dict(W=z[f"fc{k}_weight_q"], ws=z[f"fc{k}_weight_scale"], b=z[f"fc{k}_bias_q"], bs=z[f"fc{k}_bias_scale"],
                       os=s(f"fc{k}_out_scale"), oz=int(s(f"fc{k}_out_zero_point"))) for k in range(3)]
        return cls(s("input_scale"), int(s("input_zero_point")), layers, s("action_scale"), int(s("action_zero_point")))

    def arrays(self):
        """the npz key set, in the style of QuantModel's"""
        i64 = lambda v: np.full(1, int(v), np.int64)
        out = {"input_scale": np.array([self.input_scale]), "input_zero_point": i64(self.input_zero),
               "action_scale": np.array([self.action_scale]), "action_zero_point": i64(self.action_zero)}
        for k, L in enumerate(self.layers):
            out[f"fc{k}_weight_q"], out[f"fc{k}_weight_scale"] = L["W"], L["ws"]
            out[f"fc{k}_bias_q"], out[f"fc{k}_bias_scale"] = L["b"], L["bs"]
            out[f"fc{k}_out_scale"], out[f"fc{k}_out_zero_point"] = np.array([L["os"]]), i64(L["oz"])
        return out

    def save(self, path):
        np.savez(path, **self.arrays())

    # --------------------------------------------------------------------------------------------------------- contents
    def table(self):
        """the output layer's tanh table, int8 [256], indexed by q + 128 (fp64, half to even)"""
        L = self.layers[2]
        return tanh_table(L["os"], L["oz"], self.action_scale, self.action_zero)

    def float_params(self):
        """the same network with DEQUANTISED weights as the flat float32 vector in the DDPG actor's layout, W b W b W b, at the
        model's own widths (62,702 elements: what DeviceDDPGNets.act takes; 68,098 at [256, 256])"""
        parts = []
        for L in self.layers:
            parts += [(L["W"].astype(np.float64) * L["ws"][:, None]).ravel(), L["b"].astype(np.float64) * L["bs"]]
        flat = np.concatenate(parts).astype(np.float32)
        assert flat.size == ARCHS[self.net_arch].actor.count
        return flat

    def c_model(self):
        """-> (include/brs_qpolicy.h brs_qactor_model, the arrays its pointers refer to: keep them alive while it is used)"""
        m = _lib.BrsQActorModel()
        m.input_scale, m.input_zero = self.input_scale, self.input_zero
        m.action_scale, m.action_zero = self.action_scale, self.action_zero
        table = np.ascontiguousarray(self.table(), np.int8)
        keep = [table]
        for k, L in enumerate(self.layers):
            c = m.layer[k]
            c.n_in, c.n_out = L["W"].shape[1], L["W"].shape[0]
            c.weight, c.bias, c.bias_scale = L["W"].ctypes.data, L["b"].ctypes.data, L["bs"].ctypes.data
            c.out_scale, c.out_zero, c.tanh_zero = L["os"], L["oz"], 0
            c.tanh_table = table.ctypes.data if k == 2 else None
            keep += [L["W"], L["b"], L["bs"]]
        return m, keep


# what a SAC actor of another architecture's length is told, by the net_arch that was asked for
_OTHER_WIDTHS = {"reference": "this is a [256, 256] SAC actor (net_arch='sb3'): with the default net_arch the int8 actor is built at the "
                              "reference widths pi=[300, 200]; pass net_arch='sb3' to quantize_actor",
                 "sb3": "this is a SAC actor of the reference widths pi=[300, 200]: pass net_arch='reference'"}


def _actor_flat(params, head, net_arch="reference"):
    """-> the fp64 DDPG-layout actor vector of `net_arch`'s widths; with head = "sac" the mu head of a SAC actor (log_std dropped)"""
    from .offpolicy import flatten_ddpg_state_dict, flatten_sac_actor
    if head not in ("ddpg", "sac"):
        raise ValueError(f"head must be 'ddpg' or 'sac', got {head!r}")
    if net_arch not in ARCHS:
        raise ValueError(f"net_arch must be {ARCH_NAMES}, got {net_arch!r}")
    arch = ARCHS[net_arch]
    if head == "ddpg":
        if net_arch != "reference":
            raise ValueError("net_arch='sb3' is SAC's [256, 256] actor: pass head='sac' (SB3 has no DDPG or TD3 at these widths)")
        flat = flatten_ddpg_state_dict(params) if isinstance(params, dict) else np.asarray(params)
        if flat.size != arch.actor.count:
            raise ValueError(f"expected {arch.actor.count} parameters, got {flat.size}")
        return flat.astype(np.float64).ravel()
    flat = flatten_sac_actor(params) if isinstance(params, dict) else np.asarray(params)
    if any(flat.size in (other.nactor, other.nactor + 1) for other in ARCHS.values() if other is not arch):
        raise ValueError(_OTHER_WIDTHS[net_arch])
    if flat.size not in (arch.nactor, arch.nactor + 1):
        raise ValueError(f"expected {arch.nactor} (+ 1) parameters, got {flat.size}")
    flat = flat.astype(np.float64).ravel()
    # the SAC vector stacks the heads into one [4][h1] layer: mu's weights, log_std's weights, mu's bias, log_std's bias
    return np.concatenate([flat[s] for s in arch.sac_mu_slices()])


def quantize_actor(params, calibration_obs=None, head="ddpg", net_arch="reference"):
    """Post-training int8 quantisation of the off-policy actor -> QuantActorModel.  `params`: the flat DDPG_NACTOR vector
    (DeviceDDPGNets) or an SB3 / train-tool state_dict; with head = "sac" a SAC actor (flat SAC_NACTOR (+ 1) or a state_dict), of
    which the deterministic action tanh(mu(s)) is quantised and the log_std head dropped.  `calibration_obs` [k, 6] as in
    quantize_policy, whose rules hold here too: half away from zero, symmetric weights per output channel, bias_scale = input
    scale x ws, ranges from the FLOAT network in fp64 on the calibration rows.  A hidden layer's output is the POST-ReLU
    activation: range [0, max], so its zero point is always -128 (the code of real 0; a degenerate range gets scale 1).  The
    output pre-activation gets an asymmetric range; the tanh table's result has scale 1 / 128 and zero point 0.

    net_arch = "sb3" (with head = "sac"): a SAC actor at SB3's default widths [256, 256] -- flat SAC256_NACTOR (+ 1) or a state_dict
    in either naming; the rules are the same.  With the default, "reference", such an actor is refused."""
    flat = _actor_flat(params, head, net_arch)
    cal = np.asarray(REFERENCE_CALIBRATION if calibration_obs is None else calibration_obs, np.float64)
    if cal.ndim != 2 or cal.shape[1] != 6 or cal.shape[0] < 1 or not np.isfinite(cal).all():
        raise ValueError("calibration_obs: expected finite [k, 6]")
    if not np.isfinite(flat).all():
        raise ValueError("the actor's parameters are not finite")
    in_scale, in_zero = _activation_qparams(cal.min(), cal.max())
    input_scale, input_zero = in_scale, in_zero
    x, off, layers = cal, 0, []
    for k, (n_in, n_out) in enumerate(_actor_sizes(net_arch)):
        W = flat[off:off + n_in * n_out].reshape(n_out, n_in); off += n_in * n_out
        b = flat[off:off + n_out]; off += n_out
        amax = np.abs(W).max(axis=1)
        ws = np.where(amax > 0, amax / 127.0, 1.0)
        Wq = np.clip(_round_half_away(W / ws[:, None]), -127, 127).astype(np.int8)
        bs = in_scale * ws
        bq = _round_half_away(b / bs)
        if np.abs(bq).max() > 2 ** 31 - 1:
            raise ValueError(f"layer {k}: a quantised bias leaves int32 (bias {np.abs(b).max():.3g} at scale {bs.min():.3g})")
        pre = x @ W.T + b  # the float network on the calibration rows
        if k < 2:
            x = np.maximum(pre, 0.0)
            hi = float(x.max())
            os_, oz = (hi / 255.0, -128) if hi > 0.0 else (1.0, -128)
            in_scale = os_
        else:
            os_, oz = _activation_qparams(pre.min(), pre.max())
        layers.append(dict(W=Wq, b=bq.astype(np.int32), ws=ws, bs=bs, os=os_, oz=oz))
    return QuantActorModel(input_scale, input_zero, layers, 1.0 / 128.0, 0)


class QuantActor(Handle):
    """The int8 off-policy actor evaluated by the HIP kernel: obs [n, 6] -> action [n, 2], with integer arithmetic only.  The
    handle is created for the widths of `model` (model.net_arch) and serves models of those widths only."""
    _FAMILY, _WHAT = "brs_qpolicy_actor", "the int8 actor has"

    def __init__(self, model, device=0):
        self._attach(device)
        self.net_arch = model.net_arch
        self._create("brs_qpolicy_actor_create_arch", self.device.index, ARCHS[self.net_arch].id)
        self.set_model(model)

    def set_model(self, model):
        """load another QuantActorModel of the handle's widths (synchronous; takes effect on the next act)"""
        m, keep = model.c_model()
        self._check(self.L.brs_qpolicy_actor_set_model(self.h, C.byref(m)), "brs_qpolicy_actor_set_model")
        del keep
        self.model = model

    def act(self, obs, out=None, out_q=None):
        """obs [n, 6] f32 cuda -> action [n, 2] f32 (not clipped); `out_q` [n, 2] int8 receives the int8 codes"""
        n = obs.shape[0]
        d = self.device
        _need(obs, "obs", torch.float32, (n, 6), d)
        if out is None:
            out = torch.empty((n, 2), dtype=torch.float32, device=d)
        _need(out, "out", torch.float32, (n, 2), d)
        if out_q is not None:
            _need(out_q, "out_q", torch.int8, (n, 2), d)
        self._check(self.L.brs_qpolicy_actor_act(self.h, n, _p(obs), _p(out), _p(out_q), self._stream()), "brs_qpolicy_actor_act")
        return out
