"""Packed 2+2-bit I/Q input (settings.fileType 3, is_complex 2) without a GPU: the test's own packer against the reference's
look-up tables and the oracle's converter, the settings struct, the hosts' argument checks (all before any device call), and
the MEX gateway's checks for 'acquire' with iq = 2, built against a stand-in for the MEX runtime that has uint8 arrays
(tests/mex_stub_packed: tests/mex_stub plus one class)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bds_amd
from bds_amd import native
from oracle import unpack as oun

from helpers import cfg1_b2a_iq, track_case
from packed_cases import pack_iq, packed_record, quantise, uses_every_nibble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


# ---- the packer ---------------------------------------------------------------------------------------------------------
def test_pack_iq_inverts_the_reference_tables():
    lut = np.load(os.path.join(GOLD, "unpack_cplx_lut.npz"))["lut"]  # [256, 4] = I1, Q1, I2, Q2 of every byte
    assert lut.shape == (256, 4)
    np.testing.assert_array_equal(pack_iq(lut.astype(np.int8).reshape(-1)), np.arange(256, dtype=np.uint8))
    for b in range(256):  # row by row: one byte from its four values
        assert pack_iq(lut[b].astype(np.int8))[0] == b


def test_pack_iq_inverts_the_oracle_converter():
    rng = np.random.default_rng(1)
    packed = rng.integers(0, 256, 4099, dtype=np.uint8)
    pairs = oun.unpack_cplx(packed)
    np.testing.assert_array_equal(pack_iq(pairs), packed)
    np.testing.assert_array_equal(oun.unpack_cplx(pack_iq(pairs)), pairs)


def test_pack_iq_refuses_what_is_not_the_alphabet():
    with pytest.raises(ValueError):
        pack_iq(np.array([1, 3, 0, 1], dtype=np.int8))
    with pytest.raises(ValueError):
        pack_iq(np.array([1, 3], dtype=np.int8))  # one sample: half a byte
    with pytest.raises(ValueError):
        pack_iq(np.array([1.0, 3.0, 1.0, 1.0]))


def test_quantised_record_uses_the_whole_alphabet():
    s, x, _ = cfg1_b2a_iq()
    pairs = quantise(x)
    assert pairs.size == x.size // 4 * 4 and set(np.unique(pairs)) == {-3, -1, 1, 3}
    np.testing.assert_array_equal(np.sign(pairs), np.where(x[: pairs.size] < 0, -1, 1))
    # one threshold near the rms: both magnitudes are common (a Gaussian exceeds its rms 32 % of the time)
    assert 0.2 < np.mean(np.abs(pairs) == 3) < 0.45
    packed, pairs2 = packed_record(x)
    assert packed.dtype == np.uint8 and packed.size * 4 == pairs2.size and uses_every_nibble(packed)
    np.testing.assert_array_equal(oun.unpack_cplx(packed), pairs2)
    assert packed.max() > 127  # bytes an int8 conversion of VALUES would refuse or mangle
    assert not uses_every_nibble(np.zeros(64, dtype=np.uint8))


# ---- settings and host argument checks ----------------------------------------------------------------------------------
def test_pack_settings_carries_file_type_3():
    for s in (bds_amd.init_settings_b2a(fileType=3), bds_amd.init_settings_b1c(fileType=3)):
        assert native.pack_settings(s).fileType == 3


def test_sample_counts_of_the_three_formats():
    assert native.n_samples_of(10, 0) == 10 and native.n_samples_of(10, False) == 10
    assert native.n_samples_of(10, 1) == 5 and native.n_samples_of(10, True) == 5
    assert native.n_samples_of(10, 2) == 20 and native.n_samples_of(10, 2, 19) == 19  # odd: the last high nibble is ignored
    with pytest.raises(ValueError, match="holds 20 samples"):
        native.n_samples_of(10, 2, 21)
    with pytest.raises(ValueError, match="is_complex"):
        native.n_samples_of(10, 3)


class _NoDevice:
    """Stands where the context would: any use is a device call the host should not have reached."""

    def __getattr__(self, name):
        raise AssertionError(f"device call {name} before the argument check")


@pytest.fixture
def no_device(monkeypatch):
    import sys

    acq_mod, trk_mod = sys.modules[bds_amd.acquisition.__module__], sys.modules[bds_amd.tracking.__module__]
    monkeypatch.setattr(acq_mod, "get_context", lambda device=0: _NoDevice())
    monkeypatch.setattr(trk_mod, "get_context", lambda device=0: _NoDevice())


def test_hosts_refuse_sample_values_with_file_type_3(no_device):
    s, x, _ = cfg1_b2a_iq()
    s3 = s.copy(fileType=3)
    z = x[0::2].astype(np.float64) + 1j * x[1::2].astype(np.float64)
    for bad in (z, x.astype(np.float64), x.astype(np.float32)[:1000]):
        with pytest.raises(ValueError, match=r"longSignal.*fileType is 3"):
            bds_amd.acquisition(bad, s3, verbose=False)
        with pytest.raises(ValueError, match=r"longSignal.*fileType is 3"):
            bds_amd.acquire_track(bad, "/nonexistent/record.bin", s3)
    st, xt, chans = track_case("B2A", "B2A", 4, iq=True)
    for bad in (xt.astype(np.float64), xt[0::2] + 1j * xt[1::2]):
        with pytest.raises(ValueError, match=r"fid.*fileType is 3"):
            bds_amd.tracking(bad, chans, st.copy(fileType=3))


def test_an_odd_int8_array_is_no_iq_record():
    """A packed array handed over as I/Q pairs (is_complex 1) by mistake: an odd byte count cannot be pairs.  The check stands
    in front of the native call -- a context is not even needed."""
    packed = np.arange(33, dtype=np.uint8).view(np.int8)
    with pytest.raises(ValueError, match="odd count"):
        native.n_samples_of(packed.size, True)
    s = bds_amd.init_settings_b2a(fileType=2)
    ctx = native.Context.__new__(native.Context)  # no bds_create: no device
    ctx._h = None
    for call in (lambda: native.Context.acq_load(ctx, s, packed, True), lambda: native.Context.acquire(ctx, s, packed, True),
                 lambda: native.Context.acquire_track(ctx, s, packed, True, "/nonexistent", 1, 0, [])):
        with pytest.raises(ValueError, match="odd count"):
            call()


def test_uint8_bytes_reach_the_library_unchanged():
    b = np.array([0, 127, 128, 200, 255], dtype=np.uint8)
    a, _ = native._i8(b)
    assert a.dtype == np.int8
    np.testing.assert_array_equal(a.view(np.uint8), b)


# ---- the MEX gateway ----------------------------------------------------------------------------------------------------
STUB = os.path.join(ROOT, "tests", "mex_stub_packed")
SO = os.path.join(STUB, "_build", "libbds_mex_mock_packed.so")
P = ctypes.c_void_p


@pytest.fixture(scope="module")
def mex():
    """mex/bds_mex.c with its uint8 input compiled in, as tests/test_mex_mock.py builds its gateway."""
    from test_mex_mock import Mex

    pkg = os.path.dirname(native._LIB_PATH)
    libname = os.path.splitext(os.path.basename(native._LIB_PATH))[0][3:]
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-D_POSIX_C_SOURCE=200809L", "-DBDS_MEX_HAVE_UINT8", "-shared", "-fPIC",
                           "-I", STUB, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "mex", "bds_mex.c"),
                           os.path.join(STUB, "mex_mock_uint8.c"), "-L", pkg, "-l" + libname, "-Wl,-rpath," + pkg,
                           "-Wl,-rpath,/opt/rocm/lib", "-o", SO])
    L = ctypes.CDLL(SO)
    for name, res, args in [
        ("mxCreateDoubleMatrix", P, [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int]),
        ("mxCreateNumericMatrix", P, [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_int]),
        ("mxCreateStructMatrix", P, [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, P]),
        ("mxCreateString", P, [ctypes.c_char_p]), ("mxCreateLogicalScalar", P, [ctypes.c_bool]),
        ("mxAddField", ctypes.c_int, [P, ctypes.c_char_p]), ("mxSetField", None, [P, ctypes.c_size_t, ctypes.c_char_p, P]),
        ("mxGetDoubles", ctypes.POINTER(ctypes.c_double), [P]), ("mxGetInt8s", ctypes.POINTER(ctypes.c_int8), [P]),
        ("mxGetUint8s", ctypes.POINTER(ctypes.c_uint8), [P]), ("mock_create_uint8", P, [ctypes.c_size_t]),
        ("mxGetNumberOfElements", ctypes.c_size_t, [P]), ("mxDestroyArray", None, [P]),
        ("mock_call", ctypes.c_int, [ctypes.c_int, ctypes.POINTER(P), ctypes.c_int, ctypes.POINTER(P)]),
        ("mock_error_id", ctypes.c_char_p, []), ("mock_error_msg", ctypes.c_char_p, []), ("mock_run_atexit", None, []),
    ]:
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    m = Mex(L)

    def uint8(v):
        v = np.ascontiguousarray(v, dtype=np.uint8)
        a = L.mock_create_uint8(v.size)
        if v.size:
            ctypes.memmove(L.mxGetUint8s(a), v.ctypes.data, v.size)
        return a

    m.uint8 = uint8
    yield m
    L.mock_run_atexit()


def test_gateway_checks_of_the_packed_acquire(mex):
    """bds_mex('acquire', uint8 longSignal, settings, signal, 2): wrong class, no bytes, and a settings struct that does not say
    fileType 3 all leave through mexErrMsgIdAndTxt before the gateway creates its device context."""
    from test_mex_mock import MexError

    s3 = bds_amd.init_settings_b2a(fileType=3)
    packed = np.arange(64, dtype=np.uint8)
    with pytest.raises(MexError, match="uint8 longSignal of packed bytes") as e:  # wrong class: int8
        mex.call(4, mex.value("acquire"), mex.int8(packed.view(np.int8)), mex.settings(s3), mex.double(2), mex.double(2))
    assert e.value.ident == "bds:args"
    with pytest.raises(MexError, match="uint8 longSignal of packed bytes"):  # wrong class: double
        mex.call(4, mex.value("acquire"), mex.double(packed), mex.settings(s3), mex.double(2), mex.double(2))
    with pytest.raises(MexError, match="holds 0 packed bytes"):  # too short to hold a sample
        mex.call(4, mex.value("acquire"), mex.uint8(packed[:0]), mex.settings(s3), mex.double(2), mex.double(2))
    with pytest.raises(MexError, match=r"settings\.fileType = 3 go together"):
        mex.call(4, mex.value("acquire"), mex.uint8(packed), mex.settings(s3.copy(fileType=2)), mex.double(2), mex.double(2))
    with pytest.raises(MexError, match=r"settings\.fileType = 3 go together"):  # fileType 3 with int8 pairs
        mex.call(4, mex.value("acquire"), mex.int8(packed.view(np.int8)), mex.settings(s3), mex.double(2), mex.value(True))
    with pytest.raises(MexError, match="int8 longSignal"):  # a uint8 array is still no int8 record
        mex.call(4, mex.value("acquire"), mex.uint8(packed), mex.settings(s3.copy(fileType=1)), mex.double(2))
