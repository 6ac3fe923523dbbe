"""SB3's VecNormalize on the device (include/brs_policy.h: brs_vecnorm_*).

Running mean and variance of the six observation columns and of the discounted return, kept in fp64 in HBM and updated by HIP
kernels that read the simulator's outputs in place: `step` enqueues three kernels (two when the statistics are frozen: one) and
neither synchronises nor allocates, so it fits between `BatchedSim.step` and the algorithm inside `DeviceRollout.collect`.  The
reduction is a tree of fixed shape without atomics: the same inputs give the same statistics, byte for byte.

For DDPG, TD3 and SAC the object is handed to DeviceOffPolicyCollector(normalize=) and to
DeviceReplayBuffer.sample(normalize=), which normalises the minibatch inside the sampling kernel; `fold_vecnormalize` folds the
observation statistics into an actor's first layer, for deployment on raw observations."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._handle import Handle, _need, _p

_KEYS = ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count", "returns")


def fold_first_layer(w1, b1, mean, var, epsilon=1e-8):
    """the fold itself, in float64 and not yet rounded: (W1 [h][6], b1 [h]) -> (W1 / sqrt(var + epsilon) per column, b1 - W1' . mean)"""
    w = np.asarray(w1, np.float64) / np.sqrt(np.asarray(var, np.float64) + float(epsilon))
    return w, np.asarray(b1, np.float64) - w @ np.asarray(mean, np.float64)


def fold_vecnormalize(actor_flat, state_dict, net_arch="reference", epsilon=1e-8):
    """An actor trained behind a normaliser, for callers that hand it RAW observations (the int8 quantiser, a microcontroller): the
    flat float32 vector with the observation statistics of `state_dict` (DeviceVecNormalize.state_dict(), or SB3's obs_rms as
    obs_mean / obs_var) folded into the first layer,

        W1' = W1 / sqrt(var + epsilon) per column,   b1' = b1 - W1' . mean,

    computed in float64 and rounded once.  The first layer leads the flat layout of the DDPG / TD3 actor and of the SAC actor (with
    or without the trailing log_ent_coef) at both width sets; the rest of the vector is copied.  The folded actor on a raw
    observation is the original actor on the normalised one wherever no column is clipped: the clip to +-clip_obs is not linear
    and cannot be folded."""
    from . import nets
    arch = nets.arch(net_arch)
    flat = nets.flat_array(actor_flat)
    lengths = (arch.actor.count, arch.nactor, arch.nactor + 1)
    if flat.ndim != 1 or flat.shape[0] not in lengths:
        raise ValueError(f"actor_flat: expected {' or '.join(map(str, lengths))} parameters for net_arch={arch.name!r}, got shape {flat.shape}")
    for k in ("obs_mean", "obs_var"):
        if k not in state_dict:
            raise ValueError(f"state_dict: missing {k}")
    mean, var = (np.asarray(state_dict[k], np.float64).reshape(-1) for k in ("obs_mean", "obs_var"))
    if mean.shape != (6,) or var.shape != (6,):
        raise ValueError(f"state_dict: obs_mean and obs_var must hold 6 elements, got {mean.shape} and {var.shape}")
    h0 = arch.pi[0]
    w, b = fold_first_layer(flat[:6 * h0].reshape(h0, 6), flat[6 * h0:7 * h0], mean, var, epsilon)
    out = flat.copy()
    out[:6 * h0], out[6 * h0:7 * h0] = w.astype(np.float32).ravel(), b.astype(np.float32)
    return out


class DeviceVecNormalize(Handle):
    """VecNormalize for the n envs of a BatchedSim; the arguments carry SB3's names.  `training` is a plain attribute: False
    freezes the statistics (evaluation).  reset() and step() return tensors this object owns and overwrites on the next call."""
    _FAMILY, _WHAT = "brs_vecnorm", "the on-device VecNormalize has"

    def __init__(self, n, device=0, training=True, norm_obs=True, norm_reward=True, clip_obs=10., clip_reward=10., gamma=0.99,
                 epsilon=1e-8):
        self._attach(device)
        self.n, self.training = int(n), bool(training)
        self.norm_obs, self.norm_reward = bool(norm_obs), bool(norm_reward)
        self.clip_obs, self.clip_reward, self.gamma, self.epsilon = float(clip_obs), float(clip_reward), float(gamma), float(epsilon)
        cfg = _lib.BrsVecnormConfig(self.gamma, self.epsilon, self.clip_obs, self.clip_reward, int(self.norm_obs), int(self.norm_reward))
        self._create("brs_vecnorm_create", self.device.index, self.n, C.byref(cfg))
        f = lambda *s: torch.zeros(s, dtype=torch.float32, device=self.device)
        self.obs, self.reward, self.terminal_obs = f(self.n, 6), f(self.n), f(self.n, 6)

    def reset(self, obs):
        """the observations of a simulator reset [n, 6] -> normalised; the discounted returns start again at 0"""
        _need(obs, "obs", torch.float32, (self.n, 6), self.device)
        self._check(self.L.brs_vecnorm_reset(self.h, _p(obs), int(bool(self.training)), _p(self.obs), self._stream()), "brs_vecnorm_reset")
        return self.obs

    def step(self, obs, reward, terminated, truncated, terminal_obs):
        """the five arrays BatchedSim.step returned -> (obs, reward, terminal_obs) normalised with the updated statistics"""
        n, d, f32, u8 = self.n, self.device, torch.float32, torch.uint8
        _need(obs, "obs", f32, (n, 6), d); _need(reward, "reward", f32, (n,), d); _need(terminated, "terminated", u8, (n,), d)
        _need(truncated, "truncated", u8, (n,), d); _need(terminal_obs, "terminal_obs", f32, (n, 6), d)
        self._check(self.L.brs_vecnorm_step(self.h, _p(obs), _p(reward), _p(terminated), _p(truncated), _p(terminal_obs),
                                            int(bool(self.training)), _p(self.obs), _p(self.reward), _p(self.terminal_obs), self._stream()),
                    "brs_vecnorm_step")
        return self.obs, self.reward, self.terminal_obs

    def _stateless(self, call, x, tail, out):
        if not isinstance(x, torch.Tensor) or x.dim() != 1 + len(tail) or x.shape[0] < 1:
            raise ValueError(f"{call}: expected a tensor of shape {('m',) + tail} with m >= 1, got {getattr(x, 'shape', type(x))}")
        m = x.shape[0]
        _need(x, "in", torch.float32, (m,) + tail, self.device)
        if out is None:
            out = torch.empty_like(x)
        _need(out, "out", torch.float32, (m,) + tail, self.device)
        self._check(getattr(self.L, call)(self.h, m, _p(x), _p(out), self._stream()), call)
        return out

    def normalize_obs(self, obs, out=None):
        """any [m, 6] with the current statistics; no state is touched (evaluation, a replay buffer of raw observations)"""
        return self._stateless("brs_vecnorm_normalize_obs", obs, (6,), out)

    def normalize_reward(self, reward, out=None):
        return self._stateless("brs_vecnorm_normalize_reward", reward, (), out)

    def state_dict(self):
        """numpy float64: obs_mean / obs_var / obs_count [6], ret_mean / ret_var / ret_count (scalars), returns [n]; waits for
        the stream"""
        s = _lib.BrsVecnormStats()
        self._check(self.L.brs_vecnorm_get_stats(self.h, C.byref(s), self._stream()), "brs_vecnorm_get_stats")
        returns = np.zeros(self.n, np.float64)
        self._check(self.L.brs_vecnorm_get_returns(self.h, returns.ctypes.data_as(C.POINTER(C.c_double)), self._stream()),
                    "brs_vecnorm_get_returns")
        sd = {k: np.array(getattr(s, k), np.float64) for k in ("obs_mean", "obs_var", "obs_count")}
        sd.update({k: np.float64(getattr(s, k)) for k in ("ret_mean", "ret_var", "ret_count")})
        sd["returns"] = returns
        return sd

    def load_state_dict(self, sd):
        """the statistics of state_dict() (obs_count may be SB3's scalar); `returns` is not loaded: VecNormalize.load does not
        restore it either, and the next reset() zeroes it"""
        missing = [k for k in _KEYS[:6] if k not in sd]
        if missing:
            raise ValueError(f"load_state_dict: missing {missing}")
        s = _lib.BrsVecnormStats()
        for k in ("obs_mean", "obs_var", "obs_count"):
            a = np.broadcast_to(np.asarray(sd[k], np.float64), (6,))
            setattr(s, k, (C.c_double * 6)(*a.tolist()))
        for k in ("ret_mean", "ret_var", "ret_count"):
            setattr(s, k, float(np.asarray(sd[k], np.float64).reshape(())))
        self._check(self.L.brs_vecnorm_set_stats(self.h, C.byref(s), self._stream()), "brs_vecnorm_set_stats")
