"""The Python side of the library protocol (shapemol_amd/_native.py), without a GPU: pointers, host arrays, device
normalisation, the per-device context cache (against a stand-in for the library) and the loss-type table."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from shapemol_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ptr():
    assert _native.ptr(None) is None
    a = np.arange(6, dtype=np.float64)
    p = _native.ptr(a)
    assert isinstance(p, C.c_void_p) and p.value == a.ctypes.data
    t = torch.arange(6, dtype=torch.float32)
    p = _native.ptr(t)
    assert isinstance(p, C.c_void_p) and p.value == t.data_ptr()


def test_host():
    t = torch.arange(6, dtype=torch.float32).view(2, 3)
    a = _native.host(t, np.float32)
    assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == (2, 3)
    assert a.ctypes.data == t.data_ptr()                              # the dtype matches: the tensor's memory
    b = _native.host(t, np.float64)
    assert b.dtype == np.float64 and np.array_equal(b, a) and b.ctypes.data != a.ctypes.data
    c = _native.host([[1, 2], [3, 4]], np.int32)
    assert isinstance(c, np.ndarray) and c.dtype == np.int32 and c.tolist() == [[1, 2], [3, 4]]
    d = np.arange(4, dtype=np.int64)
    assert _native.host(d, np.int64) is d and _native.host(d) is d    # no copy
    assert isinstance(_native.host((1.0, 2.0)), np.ndarray)


def test_hip_device():
    with pytest.raises(RuntimeError, match="no CPU path") as e:
        _native.hip_device("cpu", "shape data is built on a HIP device")
    assert str(e.value) == "shape data is built on a HIP device (shapemol_amd has no CPU path)"
    with pytest.raises(RuntimeError, match="no CPU path"):
        _native.hip_device(torch.device("cpu"), "x")
    for given in ("cuda:1", torch.device("cuda", 1)):                 # (an index given: the current device is not asked for)
        d = _native.hip_device(given, "x")
        assert d == torch.device("cuda", 1) and d.index == 1


class _FakeLibrary:
    """Stands in for libshapemol_hip.so: create(index, &handle) and destroy(handle), with a record of both."""

    def __init__(self):
        self.created, self.destroyed, self.fail_next = [], [], False

    def fake_create(self, index, ref):
        if self.fail_next:
            self.fail_next = False
            raise RuntimeError("create failed")
        self.created.append(index)
        ref._obj.value = 1000 + 10 * index + len(self.created)       # a handle of its own for every create
        return 0

    def fake_destroy(self, handle):
        self.destroyed.append(handle.value)


@pytest.fixture
def fake(monkeypatch):
    lib = _FakeLibrary()
    monkeypatch.setattr(_native, "_lib", types.SimpleNamespace(load=lambda: lib, check=lambda rc, what: None))
    monkeypatch.setattr(_native.DeviceContexts, "_all", [])           # (the package's own caches hold real contexts: out of reach)
    return lib


def test_device_contexts(fake):
    ctxs = _native.DeviceContexts("fake_create", "fake_destroy")
    a = ctxs.of(torch.device("cuda", 0))
    assert ctxs.of("cuda:0") is a and ctxs.of(torch.device("cuda:0")) is a
    b = ctxs.of("cuda:1")
    assert ctxs.of(torch.device("cuda", 1)) is b and b is not a
    assert fake.created == [0, 1]                                     # one create per device index
    assert isinstance(a, C.c_void_p) and a.value != b.value
    handles = sorted([a.value, b.value])
    ctxs.close_all()
    assert sorted(fake.destroyed) == handles                          # each exactly once
    ctxs.close_all()
    assert sorted(fake.destroyed) == handles                          # idempotent
    c = ctxs.of("cuda:0")                                             # a closed cache creates again
    assert fake.created == [0, 1, 0] and c.value not in handles
    with pytest.raises(RuntimeError, match="no CPU path"):
        ctxs.of("cpu")


def test_device_contexts_failed_create(fake):
    ctxs = _native.DeviceContexts("fake_create", "fake_destroy")
    fake.fail_next = True
    with pytest.raises(RuntimeError, match="create failed"):
        ctxs.of("cuda:0")
    assert fake.created == [] and ctxs._by_index == {}                # nothing cached
    a = ctxs.of("cuda:0")                                             # the next call tries again
    assert fake.created == [0] and ctxs.of("cuda:0") is a
    ctxs.close_all()
    assert fake.destroyed == [a.value]


def test_device_contexts_rejected_create(monkeypatch, fake):
    """A create that returns an error code raises through _lib.check and caches nothing."""
    def check(rc, what):
        if rc:
            raise RuntimeError(f"{what} failed")
    monkeypatch.setattr(_native._lib, "check", check)
    fake.fake_create = lambda index, ref: 1
    ctxs = _native.DeviceContexts("fake_create", "fake_destroy")
    with pytest.raises(RuntimeError, match="fake_create failed"):
        ctxs.of("cuda:0")
    assert ctxs._by_index == {}
    ctxs.close_all()
    assert fake.destroyed == []


def test_one_exit_hook_closes_every_cache(fake):
    one, two = _native.DeviceContexts("fake_create", "fake_destroy"), _native.DeviceContexts("fake_create", "fake_destroy")
    a, b = one.of("cuda:0").value, two.of("cuda:0").value
    _native._close_device_contexts()
    assert sorted(fake.destroyed) == sorted([a, b])


def test_loss_types_agree_with_the_header():
    header = open(os.path.join(ROOT, "include", "shapemol_hip.h")).read()
    enum = re.search(r"enum\s*\{\s*SHAPEMOL_SD_SIGNEDDIST\s*=\s*(\d+)\s*,\s*SHAPEMOL_SD_OCCUPANCY\s*=\s*(\d+)\s*\}", header)
    assert enum, "the loss-type enum of include/shapemol_hip.h"
    assert _native.LOSS_TYPES == {"signed_distance": int(enum.group(1)), "occupancy": int(enum.group(2))}
    from shapemol_amd import shape_autoencoder, shape_data
    assert shape_data.LOSS_TYPES is _native.LOSS_TYPES and shape_autoencoder.LOSS_TYPES is _native.LOSS_TYPES


def test_get():
    assert _native.get({"a": 1}, "a") == 1 and _native.get(types.SimpleNamespace(a=2), "a") == 2
