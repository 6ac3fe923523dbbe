"""SB3's VecNormalize on the device (include/brs_policy.h: brs_vecnorm_*).

Running mean and variance of the six observation columns and of the discounted return, kept in fp64 in HBM and updated by HIP
kernels that read the simulator's outputs in place: `step` enqueues three kernels (two when the statistics are frozen: one) and
neither synchronises nor allocates, so it fits between `BatchedSim.step` and the algorithm inside `DeviceRollout.collect`.  The
reduction is a tree of fixed shape without atomics: the same inputs give the same statistics, byte for byte."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._handle import Handle, _need, _p

_KEYS = ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count", "returns")


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
