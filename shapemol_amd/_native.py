"""What every module of the package needs to call libshapemol_hip.so: pointers and streams as ctypes arguments, host arrays,
HIP devices with their index filled in, the per-device cache of library contexts, and the two lookups the shape modules share.
"""
import atexit
import ctypes as C

import numpy as np
import torch

from . import _lib

# loss_type of the shape auto-encoder's config -> the library's code (SHAPEMOL_SD_SIGNEDDIST / SHAPEMOL_SD_OCCUPANCY)
LOSS_TYPES = {"signed_distance": 0, "occupancy": 1}


def get(config, name):
    """An entry of a config given as a dict or as an attribute object."""
    return config[name] if isinstance(config, dict) else getattr(config, name)


def ptr(a):
    """A tensor's or numpy array's memory as a ``c_void_p`` argument; ``None`` stays ``None`` (a null pointer)."""
    if isinstance(a, torch.Tensor):
        return C.c_void_p(a.data_ptr())
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def stream_ptr(where):
    """A stream, or the current stream of a device, as a ``c_void_p`` argument."""
    stream = where if isinstance(where, torch.cuda.Stream) else torch.cuda.current_stream(where)
    return C.c_void_p(stream.cuda_stream)


def host(a, dtype=None):
    """A tensor or array-like as a numpy array (of ``dtype``: no copy where it has it already)."""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    return a if dtype is None else a.astype(dtype, copy=False)


def hip_device(device, what=None):
    """``torch.device('cuda', index)`` of ``device``, without an index the current one; anything but a HIP device raises
    ``RuntimeError("<what> (shapemol_amd has no CPU path)")``, ``what`` by default "<device> is not a HIP device"."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"{what or f'{device} is not a HIP device'} (shapemol_amd has no CPU path)")
    return device if device.index is not None else torch.device("cuda", torch.cuda.current_device())


def _check_device_tensor(name, t, dtype):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a tensor on a HIP device (shapemol_amd has no CPU path)")
    if t.dtype != dtype:
        raise TypeError(f"{name} must have dtype {dtype}, got {t.dtype}")
    return t.contiguous()


class DeviceContexts:
    """One library context per device, made by ``<create_name>(device index, &handle)`` at the first ``of(device)`` and
    destroyed by ``<destroy_name>(handle)`` before the interpreter tears the runtime down (not from a finaliser during it).
    Workspaces grow with the largest call seen.  A create that fails caches nothing."""
    _all = []

    def __init__(self, create_name, destroy_name):
        self.create_name, self.destroy_name = create_name, destroy_name
        self._by_index = {}
        DeviceContexts._all.append(self)

    def of(self, device):
        """The handle (a ``c_void_p``) of ``device`` (a HIP ``torch.device``)."""
        index = hip_device(device).index
        if index not in self._by_index:
            handle = C.c_void_p()
            _lib.check(getattr(_lib.load(), self.create_name)(index, C.byref(handle)), self.create_name)
            self._by_index[index] = handle
        return self._by_index[index]

    def close_all(self):
        while self._by_index:
            getattr(_lib.load(), self.destroy_name)(self._by_index.popitem()[1])


@atexit.register
def _close_device_contexts():
    for contexts in DeviceContexts._all:
        contexts.close_all()
