"""What every Python object on a handle of the C ABI shares: the refusal without a device, the library, the device, the create call
and its error, close / __del__ / _check / _stream, and the helpers that turn tensors into the raw pointers the ABI takes.

A handle family `brs_x` of include/*.h has `brs_x_destroy(h)` and `brs_x_last_error(h)` (NULL: the error of a failed create); a class
names its family in `_FAMILY` and what it is, for the refusal, in `_WHAT`, and opens the handle in two steps:

    self._attach(device)                                  # BrsError without a HIP device; then self.L and self.device
    self._create("brs_x_create", self.device.index, ...)  # the out-pointer is appended; BrsError with the family's text; self.h
"""
import ctypes as C

import numpy as np
import torch

from . import _lib


class BrsError(RuntimeError):
    pass


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _need(t, name, dtype, shape, device):
    """the C ABI takes raw pointers: a sliced, float64 or host tensor would be read as garbage without any error"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != device:
        raise ValueError(f"{name}: expected a tensor on {device}, got {getattr(t, 'device', type(t))}")
    if t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected contiguous {dtype} of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)} "
                         f"(contiguous: {t.is_contiguous()})")
    return t


def _device(device):
    """int, 'cuda:1' or torch.device -> torch.device('cuda', index)"""
    return torch.device("cuda", device if isinstance(device, int) else torch.device(device).index or 0)


def _numpy(a):
    """a tensor (wherever it lives) or anything array-like -> numpy"""
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


class DeviceObject:
    """an object that launches kernels of the library on one device"""
    _WHAT = None   # subject and verb of the refusal: "the on-device policy has"

    def _attach(self, device):
        if not torch.cuda.is_available():
            raise BrsError(f"no HIP device visible to PyTorch: {self._WHAT} no CPU fallback")
        self.L = _lib.lib()
        self.device = _device(device)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)


class Handle(DeviceObject):
    """a DeviceObject that owns one handle `h` of the family `_FAMILY`"""
    _FAMILY = None

    def _create(self, create, *args):
        h = C.c_void_p()
        rc = getattr(self.L, create)(*args, C.byref(h))
        if rc != 0:
            raise BrsError(f"{create} failed ({rc}): {self._last_error(None)}")
        self.h = h

    def _last_error(self, h):
        return getattr(self.L, self._FAMILY + "_last_error")(h).decode()

    def close(self):
        if getattr(self, "h", None):
            getattr(self.L, self._FAMILY + "_destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise BrsError(f"{what} failed ({rc}): {self._last_error(self.h)}")
