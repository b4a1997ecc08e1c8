"""16-bit records without a GPU: the record builders of tests/int16_cases.py, settings.dataType in pack_settings, the routing of an
array by its dtype together with the setting, and -- on the float64 oracle -- the scaling claim the GPU tests lean on: a record
of 256 x8 gives exactly 256 x the correlator sums of x8 and bit-equal scale-free outputs."""
import sys

import numpy as np
import pytest

import bds_amd
from bds_amd import native
from oracle import tracking as otrk

from int16_cases import CORR_FIELDS, N_EXTREMES, assert_scaled_results, case, embed, full, scale, settings16


def test_builders():
    rng = np.random.default_rng(1)
    x8 = rng.integers(-128, 128, 4096, dtype=np.int8)
    x8[:2] = (-128, 127)
    e, sc, fu = embed(x8), scale(x8), full(x8)
    assert e.dtype == sc.dtype == fu.dtype == np.int16
    np.testing.assert_array_equal(e, x8)  # the same values
    np.testing.assert_array_equal(sc.astype(np.int64), 256 * x8.astype(np.int64))  # exact, the ends of the range included
    assert sc.min() == -32768 and sc.max() == 127 * 256
    assert np.count_nonzero(fu == -32768) >= N_EXTREMES // 2 and np.count_nonzero(fu == 32767) >= N_EXTREMES // 2
    ordinary = (fu != -32768) & (fu != 32767)
    assert not np.any(fu[ordinary].astype(np.int64) % 256 == 0)  # no multiple of 256 but the samples set to -32768
    assert np.abs(fu.astype(np.int64) - 256 * x8.astype(np.int64))[ordinary].max() <= 128
    low = (fu.view(np.uint16) & 0xFF)[ordinary]
    assert len(np.unique(low)) > 200  # the low byte carries bits of its own
    np.testing.assert_array_equal(full(x8), fu)  # seeded


@pytest.mark.parametrize("name,code", [("schar", 0), ("int8", 0), ("int16", 1), ("short", 1), ("float32", native.DATA_TYPE_REFUSED),
                                       ("uint16", native.DATA_TYPE_REFUSED), ("double", native.DATA_TYPE_REFUSED)])
def test_pack_settings_data_type(name, code):
    s = bds_amd.init_settings_b2a()
    assert native.pack_settings(s.copy(dataType=name)).dataType == code
    assert native.DATA_TYPE_REFUSED not in (0, 1)


def test_routing_by_dtype_and_setting():
    s8 = bds_amd.init_settings_b2a()
    s16 = settings16(s8)
    a8, a16 = np.arange(-4, 4, dtype=np.int8), np.array([-32768, -1, 0, 258, 32767, 5], dtype=np.int16)
    b, w16 = native.record_bytes(s8, a8)
    assert not w16 and b.dtype == np.int8 and np.array_equal(b, a8)
    b, w16 = native.record_bytes(s16, a16)
    assert w16 and b.dtype == np.int8 and b.size == 2 * a16.size
    np.testing.assert_array_equal(b.view("<i2"), a16)  # the bytes of the samples, little-endian
    assert np.shares_memory(b, a16)  # (no copy of a contiguous int16 array)
    np.testing.assert_array_equal(native.record_bytes(s16, a16.astype(">i2"))[0].view("<i2"), a16)  # (big-endian in memory: converted)
    # values of another dtype are converted under the setting
    np.testing.assert_array_equal(native.record_bytes(s16, a16.astype(np.float64))[0].view("<i2"), a16)
    with pytest.raises(ValueError, match="int16 values"):
        native.record_bytes(s16, np.array([40000.0]))
    # a disagreement names dataType, in both directions, for host arrays and for the dtype of a device array
    for settings, arr in ((s8, a16), (s16, a8), (s16, a8.view(np.uint8))):
        with pytest.raises(native.BdsError, match="dataType"):
            native.record_bytes(settings, arr)
        with pytest.raises(native.BdsError, match="dataType"):
            native.record_is_int16(settings, arr.dtype.name)
    with pytest.raises(native.BdsError, match="dataType"):
        sys.modules["bds_amd.acquisition"]._as_int8(a16, s8)  # what acquisition() does with a host array, before any copy
    assert native.record_is_int16(s16, "int16") and not native.record_is_int16(s8, "int8")
    assert not native.record_is_int16(s8.copy(dataType="float32"), "int8")  # (left to the library, which refuses the setting)


def test_feed_bytes_of_a_16_bit_session():
    sess = {"feed": True, "fileType": 2, "w16": True}
    a16 = np.array([1, -2, 300, -32768], dtype=np.int16)
    np.testing.assert_array_equal(native.check_feed_bytes(sess, a16).view("<i2"), a16)
    raw = a16.view(np.uint8)[:3]  # raw bytes in a piece that splits a sample
    assert native.check_feed_bytes(sess, raw).size == 3
    native.check_feed_span(sess, 3)
    with pytest.raises(native.BdsError, match="dataType"):
        native.check_feed_bytes(sess, np.zeros(4, dtype=np.int8))
    with pytest.raises(native.BdsError, match="dataType"):
        native.check_feed_bytes({"feed": True, "fileType": 1, "w16": False}, a16)


@pytest.mark.parametrize("signal,mode,n_epochs", [("B2A", "B2A", 20), ("B1C", "WB", 10)])
def test_oracle_scaling(signal, mode, n_epochs):
    """The reference side of the scaling claim: the oracle on scale(x8) (an int16 array: RawFile addresses elements) against the
    oracle on x8."""
    s, s16, x8, chans = case(signal, mode, n_epochs)
    t8, t16 = [], []
    want, _ = otrk.tracking(otrk.RawFile(x8), chans, s, mode=mode, trace=t8)
    got, _ = otrk.tracking(otrk.RawFile(scale(x8)), chans, s16, mode=mode, trace=t16)
    assert len(t8) == len(t16) == n_epochs * len(chans)
    for a, b in zip(t8, t16):
        np.testing.assert_array_equal(np.asarray(b["sums"]), 256.0 * np.asarray(a["sums"]))
        assert (a["pos"], a["blk"], a["rem"], a["codeFreq"], a["remCarr"], a["carrFreq"]) == (b["pos"], b["blk"], b["rem"], b["codeFreq"], b["remCarr"], b["carrFreq"])
    for g, w in zip(got, want):
        assert g.status == w.status == "T"
        for f in ("carrFreq", "codeFreq", "absoluteSample", "remCodePhase", "remCarrPhase"):
            np.testing.assert_array_equal(getattr(g, f), getattr(w, f), err_msg=f)
    assert_scaled_results(got, want)  # every field: the correlator outputs x 256, discriminators, C/N0 and lock detector bit-equal
    assert all(hasattr(want[0], f) for f in CORR_FIELDS[:8])
