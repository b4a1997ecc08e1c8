"""native.device_span / is_device_array: what the Python layer accepts as a record in device memory, checked without a GPU.

The device arrays here are mocks: an object with __cuda_array_interface__ whose pointer is that of a torch tensor in HOST memory.
device_span is a pure function -- it reads the interface and never dereferences the pointer -- so the pointer arithmetic of slices
and views is checked on real torch storage, and every refusal is seen to come before any native call (the library is not even
loaded by these tests)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from bds_amd import native


class FakeDeviceArray:
    """A torch tensor in host memory behind the interface a device array shows (strides given only when not contiguous, as the
    protocol has it); .device tells the ordinal like cupy's (an object with .id)."""

    def __init__(self, t, device=0, always_strides=False):
        self.t = t
        self.device = type("Dev", (), {"id": device})() if device is not None else None
        self.always_strides = always_strides

    @property
    def __cuda_array_interface__(self):
        t = self.t
        item = t.element_size()
        strides = None if (t.is_contiguous() and not self.always_strides) else tuple(int(s) * item for s in t.stride())
        typestr = {torch.int8: "|i1", torch.uint8: "|u1", torch.float64: "<f8", torch.int16: "<i2", torch.float32: "<f4"}[t.dtype]
        return {"shape": tuple(t.shape), "typestr": typestr, "data": (t.data_ptr(), False), "version": 3, "strides": strides}


@pytest.fixture(autouse=True)
def no_native_call(monkeypatch):
    """Every case below must be decided without the library: loading it fails the test."""
    def boom():
        raise AssertionError("device_span reached for the native library")
    monkeypatch.setattr(native, "lib", boom)


def test_a_cpu_tensor_is_refused():
    t = torch.zeros(64, dtype=torch.int8)
    assert not native.is_device_array(t)  # (it takes the host entries, as a NumPy array does)
    with pytest.raises(TypeError, match="host memory"):
        native.device_span(t, 0)
    with pytest.raises(TypeError, match="not a device array"):
        native.device_span(np.zeros(64, dtype=np.int8), 0)
    with pytest.raises(TypeError, match="not a device array"):
        native.device_span("record.bin", 0)


def test_a_non_contiguous_array_is_refused():
    base = torch.zeros((8, 16), dtype=torch.int8)
    for view in (base[:, ::2], base.t(), base[::2]):
        a = FakeDeviceArray(view)
        assert native.is_device_array(a)
        with pytest.raises(ValueError, match="not contiguous"):
            native.device_span(a, 0)
    # contiguous with the strides spelt out, and a length-1 axis whose stride does not matter
    assert native.device_span(FakeDeviceArray(base, always_strides=True), 0)[1] == 128
    assert native.device_span(FakeDeviceArray(base[:1, :], always_strides=True), 0)[1] == 16


@pytest.mark.parametrize("dtype", [torch.int16, torch.float32, torch.float64])
def test_a_wrong_dtype_is_refused(dtype):
    a = FakeDeviceArray(torch.zeros(32, dtype=dtype))
    with pytest.raises(TypeError, match="int8 / uint8"):
        native.device_span(a, 0)


def test_the_generators_clean_format_takes_float64_only():
    f = FakeDeviceArray(torch.zeros(32, dtype=torch.float64))
    assert native.device_span(f, 0, dtypes=("float64",))[1] == 256
    with pytest.raises(TypeError, match="float64"):
        native.device_span(FakeDeviceArray(torch.zeros(32, dtype=torch.int8)), 0, dtypes=("float64",))


def test_a_wrong_device_index_is_refused():
    a = FakeDeviceArray(torch.zeros(32, dtype=torch.int8), device=1)
    with pytest.raises(ValueError, match="device 1.*device 0"):
        native.device_span(a, 0)
    assert native.device_span(a, 1)[1] == 32
    # an array that tells no device is left to the library's pointer rule
    assert native.device_span(FakeDeviceArray(torch.zeros(32, dtype=torch.int8), device=None), 3)[1] == 32


def test_pointer_and_byte_count_of_a_slice_at_offset_5():
    base = torch.arange(100, dtype=torch.int8)
    a = FakeDeviceArray(base[5:77])
    ptr, n_bytes, keep = native.device_span(a, 0)
    assert ptr == base.data_ptr() + 5 and n_bytes == 72 and keep is a
    assert ptr % 2 == (base.data_ptr() + 1) % 2  # (any byte alignment is accepted)


def test_pointer_and_byte_count_of_a_uint8_view():
    base = torch.arange(100, dtype=torch.int8)
    view = base.view(torch.uint8)[10:]
    ptr, n_bytes, _ = native.device_span(FakeDeviceArray(view), 0)
    assert ptr == base.data_ptr() + 10 and n_bytes == 90
    pairs = torch.zeros((50, 2), dtype=torch.int8)  # I/Q pairs as a 2-D array: one run of 100 bytes
    ptr, n_bytes, _ = native.device_span(FakeDeviceArray(pairs), 0)
    assert ptr == pairs.data_ptr() and n_bytes == 100
    f64 = torch.zeros(40, dtype=torch.float64)[3:]
    ptr, n_bytes, _ = native.device_span(FakeDeviceArray(f64), 0, dtypes=("float64",))
    assert ptr == f64.data_ptr() and n_bytes == 37 * 8


def test_an_empty_array_is_a_null_span():
    ptr, n_bytes, _ = native.device_span(FakeDeviceArray(torch.zeros(0, dtype=torch.int8)), 0)
    assert (ptr, n_bytes) == (0, 0)


def test_feed_checks_of_a_device_span():
    with pytest.raises(ValueError, match="reads its record itself"):
        native.check_feed_span({"feed": False, "fileType": 1}, 64)
    with pytest.raises(ValueError, match="whole int8 pairs"):
        native.check_feed_span({"feed": True, "fileType": 2}, 63)
    native.check_feed_span({"feed": True, "fileType": 2}, 64)
    native.check_feed_span({"feed": True, "fileType": 3}, 63)


def test_routing_is_by_type():
    assert native.is_device_array(FakeDeviceArray(torch.zeros(4, dtype=torch.int8)))
    for host in (np.zeros(4, dtype=np.int8), torch.zeros(4, dtype=torch.int8), b"abc", "path", [1, 2, 3], None):
        assert not native.is_device_array(host)


# ---- header and mirror -----------------------------------------------------------------------------------------------------
def test_every_device_entry_of_the_header_is_exported_and_has_a_context_method():
    """The five entries are declared (BDS_DEV_API) below the text that states their contract, the built library exports each, and
    native.Context has the method of the same name."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "bds_mi355x.h")).read()
    declared = sorted(set(re.findall(r"BDS_DEV_API\s+[\w\s\*]+?\b(bds_\w+)\s*\(", src)))
    assert declared == sorted(native.DEVICE_EXPORTS) and len(declared) == 5
    assert not set(declared) & set(native.EXPORTS)
    built = ctypes.CDLL(native._LIB_PATH)  # (symbols only: no entry is called)
    contract = src[: src.index("#define BDS_DEV_API")]
    for entry in declared:
        assert hasattr(built, entry), entry
        assert callable(getattr(native.Context, entry[4:])), entry  # bds_synth_dev -> Context.synth_dev
        assert re.search(r"\b%s\b" % entry, contract), entry
    for rule in ("pointer rule", "ordering rule", "hipPointerGetAttributes", "hipMemGetAddressRange", "until bds_track_close"):
        assert rule in contract, rule
