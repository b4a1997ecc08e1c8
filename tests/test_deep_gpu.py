"""Weak-signal acquisition on the GPU (bds_acq_deep) against the NumPy float64 model of tests/deep_cases.py.

Every accumulated surface value is held to 2e-5 sum_k (max m_k)^2 of its PRN -- the 1e-5-of-the-maximum budget of the fp32-storage
search (GRID_TOL[0] of tests/test_acq_gpu.py), doubled by the square; the cell, codePhase and carrFreq are exact (the scenes' model
margins are asserted in tests/test_deep_cases.py), deepMetric within the bound that tolerance propagates to, the fine sums within
1e-9 of their maximum.  Measured worst ratios: profiles/deep_errors.txt."""
import numpy as np
import pytest

import bds_amd
import deep_cases as dc
from bds_amd import native
from oracle import acquisition as oacq

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["small_b2a", "small_b1c", "small_b1c_nopilot", "wrap_b2a"])
def test_surface_values(ctx, name):
    """All D x N values of every PRN's surface.  wrap_b2a: shifts of -1, 0 and +1 samples, rows that wrap around both ends."""
    if name == "wrap_b2a":
        s, _, k = dc.wrap_b2a()
        sh = dc.shifts(s, k)
        assert sh.min() == -1 and sh.max() == 1
    for prn, ratio in dc.surface_errors(name).items():
        print(f"\ndeep_errors: {name} PRN {prn} worst |error| / tolerance = {ratio:.3e}")
        assert ratio <= 1.0, (name, prn, ratio)


def _check_against_model(got, m, ctx):
    for prn, r in m.items():
        i = prn - 1
        assert got.fbin[i] == r.fbin, prn
        assert abs(got.deepMetric[i] - r.deepMetric) <= dc.deep_metric_bound(r), (prn, got.deepMetric[i], r.deepMetric)
        np.testing.assert_allclose(got.peakMetric[i], r.peakMetric, rtol=1e-4)
        if r.detected:
            assert got.codePhase[i] == r.codePhase and got.carrFreq[i] == r.carrFreq, prn
            f = ctx.acq_deep_fine(prn)
            assert f.shape == r.F.shape and np.max(np.abs(f - r.F)) <= 1e-9 * r.F.max(), prn
        else:
            assert got.codePhase[i] == 0 and got.carrFreq[i] == 0 and ctx.acq_deep_fine(prn).size == 0, prn


def test_detects_what_acquisition_misses_b2a(ctx):
    """PRN 9 at 46 dB-Hz, PRN 14 at 36 dB-Hz, PRN 21 absent: acquisition finds 9 only, 16 blocks find 9 and 14 and reject 21."""
    s, x, k = dc.mixed_b2a()
    ref = bds_amd.acquisition(x, s, verbose=False)
    assert [bool(c) for c in ref.carrFreq[[8, 13, 20]]] == [True, False, False]
    got = bds_amd.acquisition_deep(x, s, k, dc.THRESHOLD)
    m = dc.scene_model("mixed_b2a")
    assert [m[p].detected for p in (9, 14, 21)] == [True, True, False]
    assert [bool(c) for c in got.carrFreq[[8, 13, 20]]] == [True, True, False]
    assert (got.fbin[13], got.codePhase[13]) == (8, 20323)
    _check_against_model(got, m, ctx)
    ch = bds_amd.pre_run(got, s)  # the result feeds preRun unchanged
    assert sorted(c.PRN for c in ch if c.PRN) == [9, 14]


def test_detects_what_acquisition_misses_b1c(ctx):
    """A 35 dB-Hz B1C satellite: below acqThreshold for acquisition, found by 8 blocks; the absent PRN stays out."""
    s, x, k = dc.mixed_b1c()
    ref = bds_amd.acquisition(x, s, verbose=False)
    assert not ref.carrFreq.any()
    got = bds_amd.acquisition_deep(x, s, k, dc.THRESHOLD)
    m = dc.scene_model("mixed_b1c")
    assert m[12].detected and not m[7].detected
    assert got.carrFreq[11] != 0 and got.carrFreq[6] == 0
    _check_against_model(got, m, ctx)


@pytest.mark.parametrize("scene", ["mixed_b2a", "mixed_b1c"])
def test_one_block_is_acquisition(ctx, scene):
    """K = 1 on the record acquisition searched: the same cell, peakMetric within 2e-5 relative."""
    s, x, _ = dc.GPU_SCENES[scene]()
    bds_amd.acquisition(x, s, verbose=False)
    pk, dn, fb = ctx.acq_peaks(max(s.acqSatelliteList))
    diag = {}
    ref = oacq.acquisition(dc.as_samples(x, s), s, diag)
    got = bds_amd.acquisition_deep(x, s, 1, dc.THRESHOLD)
    for p in s.acqSatelliteList:
        assert got.fbin[p - 1] == fb[p - 1] == diag[p]["fbin"]
        np.testing.assert_allclose(got.peakMetric[p - 1], pk[p - 1] / dn[p - 1], rtol=2e-5)
        np.testing.assert_allclose(got.peakMetric[p - 1], ref.peakMetric[p - 1], rtol=2e-5)
        if got.codePhase[p - 1]:
            assert got.codePhase[p - 1] == diag[p]["codePhase"]


def _fields(r):
    return np.concatenate([r.carrFreq, r.codePhase, r.peakMetric, r.deepMetric, r.fbin.astype(np.float64)]).tobytes()


@pytest.mark.parametrize("iq", [False, True])
def test_input_and_group_invariance(ctx, iq):
    """The same bits from a host array and a tensor in HBM, from one PRN group and one PRN per group, and from two runs -- on the real
    record and on an I/Q record (iq_sign = -1), whose results also meet the model; and the real record handed over as I/Q pairs
    with Q = 0 takes the I/Q path to the bits of the real path."""
    import torch

    s, raw, k = dc.mixed_b2a(iq)
    x = dc.as_samples(raw, s) if iq else raw  # (a host I/Q record is handed over as complex values, a tensor as its int8 pairs)
    a = bds_amd.acquisition_deep(x, s, k, dc.THRESHOLD)
    assert _fields(a) == _fields(bds_amd.acquisition_deep(x, s, k, dc.THRESHOLD))
    assert _fields(a) == _fields(bds_amd.acquisition_deep(torch.from_numpy(np.array(raw)).cuda(), s, k, dc.THRESHOLD))
    _, _, n, _ = dc.sizes(s)
    one = 11 * n * 4 * 1.5 / 2 ** 30  # room for one PRN's surface, not for two
    assert _fields(a) == _fields(bds_amd.acquisition_deep(x, s, k, dc.THRESHOLD, surface_gib=one))
    with pytest.raises(native.BdsError, match="keep_surface"):
        bds_amd.acquisition_deep(x, s, k, dc.THRESHOLD, surface_gib=one, keep_surface=True)
    if iq:
        m = dc.model(raw, s, k, dc.THRESHOLD)
        assert [m[p].detected for p in (9, 14, 21)] == [True, True, False] and min(r.margin / r.tol for r in m.values()) > 100
        _check_against_model(a, m, ctx)
    else:
        assert _fields(a) == _fields(bds_amd.acquisition_deep(x.astype(np.complex128), s.copy(fileType=2), k, dc.THRESHOLD))


def test_refusals_write_nothing(ctx):
    """Packed, int16 and resampling inputs: BDS_ERR_UNSUPPORTED (-3); a short record, K = 0, threshold <= 1: BDS_ERR_ARG (-1).  The
    result arrays keep the caller's bytes in every case."""
    import ctypes as C

    s, x, k = dc.small_b2a()
    x = np.array(x)
    lib, cs = native.lib(), native.pack_settings(s)
    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)

    def call(cs, buf, n, fmt, k, thr):
        d = [np.full(14, 7.5) for _ in range(4)]
        i = [np.full(14, 7, dtype=np.int32) for _ in range(2)]
        o = native.DeepOpts(k, 1, 0, thr, 0.0)
        rc = lib.bds_acq_deep(ctx._h, C.byref(cs), buf.ctypes.data_as(C.POINTER(C.c_int8)), n, fmt, C.byref(o), 14,
                              *[a.ctypes.data_as(DP) for a in d], *[a.ctypes.data_as(IP) for a in i])
        assert all((a == 7.5).all() for a in d) and all((a == 7).all() for a in i)
        return rc

    assert call(cs, x, x.size, 2, k, 1.5) == -3                                     # packed bytes
    assert call(native.pack_settings(s.copy(dataType="int16")), x, x.size // 2, 0, k, 1.5) == -3
    assert call(native.pack_settings(s.copy(resamplingflag=1, resamplingThreshold=20e6)), x, x.size, 0, k, 1.5) == -3
    assert call(cs, x, 5 * 25000 - 1, 0, k, 1.5) == -1                              # N + K spc = 5 spc
    assert call(cs, x, x.size, 0, 0, 1.5) == -1
    assert call(cs, x, x.size, 0, k, 1.0) == -1
    assert call(cs, x, x.size, 0, k, float("nan")) == -1
    assert call(cs, x, x.size, 0, k, -2.0) == -1
