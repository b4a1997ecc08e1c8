"""Weak-signal acquisition on the GPU (bds_acq_deep) against the NumPy float64 model of tests/deep_cases.py.

Every accumulated surface value is held to 2e-5 sum_k (max m_k)^2 of its PRN -- the 1e-5-of-the-maximum budget of the fp32-storage
search (GRID_TOL[0] of tests/test_acq_gpu.py), doubled by the square; the cell, codePhase and carrFreq are exact (the scenes' model
margins are asserted in tests/test_deep_cases.py), deepMetric within the bound that tolerance propagates to, the fine sums within
1e-9 of their maximum.  Measured worst ratios: profiles/deep_errors.txt.

The surface runs write into surfaces that hold another record's values (deep_cases.run_scene_on_stale_surfaces): the library never
zeroes a surface, and a value the column pass did not write must not pass for right.  Beyond the plain scenes: shifts of 2 samples
and of a whole code period less 2, compensate = 0, peaks at both ends of the surface (clipped second-peak ranges), the
single-component B1C path and I/Q B1C records, the bin-chunk loop with b0 > 0, uneven PRN groups, the refusals.  The column pass on
multi-wave plans: tests/test_deep_plans_gpu.py."""
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


def _surface_within_tolerance(name, compensate=True):
    for prn, ratio in dc.surface_errors(name, compensate).items():
        print(f"\ndeep_errors: {name}{'' if compensate else ' compensate = 0'} PRN {prn} worst |error| / tolerance = {ratio:.3e}")
        assert ratio <= 1.0, (name, prn, ratio)


def test_shifts_of_two_samples_and_none_b2a(ctx):
    """drift_b2a: +-14 kHz over 16 blocks moves the rows by up to 2 samples, by a non-zero amount at both detected bins.  With the
    alignment and without it (compensate = 0: never a shift, other cells, lower deepMetric) the run meets its own model; without it
    every surface value as well."""
    s, _, k = dc.drift_b2a()
    sh = dc.shifts(s, k)
    assert sorted(set(sh.ravel())) == [-2, -1, 0, 1, 2]
    m, m0 = dc.scene_model("drift_b2a"), dc.scene_model("drift_b2a", False)
    assert (m[9].fbin, m[14].fbin) == (15, 1) and sh[k - 1, 14] == 2 and sh[k - 1, 0] == -2
    assert all(r.detected for r in m.values()) and all(r.detected for r in m0.values())
    assert [m[p].codePhase for p in (9, 14)] != [m0[p].codePhase for p in (9, 14)] and all(m0[p].deepMetric < m[p].deepMetric for p in (9, 14))
    assert min(r.margin / r.tol for r in m0.values()) > 100
    _check_against_model(dc.run_scene("drift_b2a", keep_surface=False), m, ctx)
    _surface_within_tolerance("drift_b2a", compensate=False)
    _check_against_model(dc.run_scene("drift_b2a", keep_surface=False, compensate=False), m0, ctx)


def test_shifts_up_to_a_code_period_b2a(ctx):
    """shift_b2a (carrFreqBasis = 6001 Hz, unphysical by design): sh from -(spc - 2) to spc - 2, the whole range the library takes;
    every surface value -- each row added at (l + sh) mod N, over both wraps."""
    s, _, k = dc.shift_b2a()
    sh = dc.shifts(s, k)
    assert (sh.min(), sh.max()) == (-11998, 11998) == (2 - dc.sizes(s)[0], dc.sizes(s)[0] - 2)
    _surface_within_tolerance("shift_b2a")


@pytest.mark.parametrize("name", sorted(dc.EDGES))
def test_peak_at_an_end_of_the_surface_b2a(ctx, name):
    """The peak in the first / last lags: the second-peak ranges of peakMetric (B2a/acquisition.m:224-249) are clipped -- the left one
    empty, the right one cut at N -- or the peak is the image in the second code period.  Each scene meets the cases its name says;
    together all three.  The records have exactly N + K spc samples."""
    s, x, k = dc.edge_b2a(name)
    spc, _, n, _ = dc.sizes(s)
    assert x.size == n + k * spc
    m = dc.scene_model(name)
    want = {"edge_b2a_left": (True, False, False), "edge_b2a_first": (True, False, False), "edge_b2a_image": (False, False, True),
            "edge_b2a_right": (False, True, True)}
    assert m[9].detected and dc.edge_conditions(s, m[9].codePhase) == want[name], (m[9].codePhase, want[name])
    assert [any(w[i] for w in want.values()) for i in range(3)] == [True] * 3
    _check_against_model(dc.run_scene(name, keep_surface=False), m, ctx)


@pytest.mark.parametrize("name", ["coh10_b1c_nopilot", "coh10_b1c_iq", "coh10_b1c_nopilot_iq"])
def test_single_component_and_iq_records_b1c(ctx, name):
    """B1C with acqCohT = 10: the single-component decision and k_deep_fine<1> (pilotACQflag = 0), and the normaliser of peakMetric
    (k_deep_sigpow) on I/Q pairs, with the pilot and without."""
    m = dc.scene_model(name)
    assert m[12].detected and (m[12].fbin, m[12].codePhase) == (4, 31004)
    _check_against_model(dc.run_scene(name, keep_surface=False), m, ctx)


def test_bin_chunks(ctx, capfd):
    """201 bins on a forced 1280 x 324 plan: the inter-pass buffer (2^30 bytes) takes Dc = 161 bins of the two components, so every
    block's bin loop runs twice, the second time with b0 = Dc > 0 in the signal loader, the surface rows and the shifts.  The rows
    around the chunk boundary, the first and the last, and the peak's row (in the second chunk) with its neighbours, value by value;
    the decision against the model."""
    s, _, k = dc.chunks_b2a()
    _, x_len, n, _ = dc.sizes(s)
    l1, l2, nc = 1280, 324, 2
    d = len(oacq.freq_bins(s))
    d_chunk = 2 ** 30 // (8 * l1 * l2 * nc)
    assert d == 201 and d_chunk == 161 and 1 < d_chunk < d
    r = dc.scene_model("chunks_b2a")[9]
    assert r.detected and d_chunk + 2 < r.fbin < d
    with dc.verbose_plans(ctx):  # (releases the 2 GiB afterwards)
        capfd.readouterr()
        got = dc.run_scene_on_stale_surfaces("chunks_b2a", f"{l1}x{l2}")
        assert dc.plans_that_ran(capfd.readouterr().err) == [(n + x_len - 1, 9, 4096), (n + x_len - 1, l1, l2)]
        worst = 0.0
        for b in sorted({1, d_chunk - 1, d_chunk, d_chunk + 1, d_chunk + 2, d, r.fbin - 1, r.fbin, r.fbin + 1}):  # 1-based
            row = ctx.acq_deep_row(9, b, n).astype(np.float64)
            ratio = float(np.max(np.abs(row - r.surface[b - 1]))) / r.tol
            worst = max(worst, ratio)
            assert ratio <= 1.0, (b, ratio)
        print(f"\ndeep_errors: chunks_b2a plan {l1} x {l2} PRN 9 worst |error| / tolerance = {worst:.3e}")
        _check_against_model(got, {9: r}, ctx)


def test_uneven_prn_groups(ctx):
    """Three PRNs with room for two surfaces: groups of 2 and 1 (np < PG in the last) give the bytes of the single group."""
    s, x, k = dc.mixed_b2a()
    _, _, n, _ = dc.sizes(s)
    two = 11 * n * 4 * 2.5 / 2 ** 30  # room for two PRNs' surfaces, not for three
    assert _fields(bds_amd.acquisition_deep(x, s, k, dc.THRESHOLD)) == _fields(bds_amd.acquisition_deep(x, s, k, dc.THRESHOLD, surface_gib=two))


def test_row_fine_and_release(ctx):
    """acq_deep_row needs a kept surface: it raises after a run without one and after the release; acq_deep_fine raises for a PRN the
    last call did not search; a second release is harmless and the next run starts from nothing."""
    s, _, _ = dc.plans_b2a()
    _, _, n, _ = dc.sizes(s)
    dc.run_scene("plans_b2a", keep_surface=False)
    with pytest.raises(native.BdsError, match="no surface is kept"):
        ctx.acq_deep_row(9, 1, n)
    with pytest.raises(native.BdsError, match="PRN 21 was not searched"):
        ctx.acq_deep_fine(21)
    dc.run_scene("plans_b2a")
    assert ctx.acq_deep_row(9, 1, n).shape == (n,) and ctx.acq_deep_fine(9).size == 21
    for bad in ((21, 1), (9, 0), (9, 10)):
        with pytest.raises(native.BdsError, match="not in the last call's grid"):
            ctx.acq_deep_row(*bad, n)
    with pytest.raises(native.BdsError, match="a row has 24000"):
        ctx.acq_deep_row(9, 1, n - 1)
    ctx.acq_deep_release()
    with pytest.raises(native.BdsError, match="no surface is kept"):
        ctx.acq_deep_row(9, 1, n)
    with pytest.raises(native.BdsError, match="no call yet"):
        ctx.acq_deep_fine(9)
    ctx.acq_deep_release()
    m = dc.scene_model("plans_b2a")
    _check_against_model(dc.run_scene("plans_b2a", keep_surface=False), m, ctx)


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
    """Packed, int16 and resampling inputs: BDS_ERR_UNSUPPORTED (-3); a short record, K = 0, K = 4097, threshold <= 1, result
    arrays shorter than the list's top PRN, a code drift of a whole period: BDS_ERR_ARG (-1).  The result arrays keep the caller's
    bytes in every case."""
    import ctypes as C

    s, x, k = dc.small_b2a()
    x = np.array(x)
    lib, cs = native.lib(), native.pack_settings(s)
    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)

    def call(cs, buf, n, fmt, k, thr, max_prn=14):
        d = [np.full(14, 7.5) for _ in range(4)]
        i = [np.full(14, 7, dtype=np.int32) for _ in range(2)]
        o = native.DeepOpts(k, 1, 0, thr, 0.0)
        rc = lib.bds_acq_deep(ctx._h, C.byref(cs), buf.ctypes.data_as(C.POINTER(C.c_int8)), n, fmt, C.byref(o), max_prn,
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
    assert call(cs, x, x.size, 0, 4097, 1.5) == -1 and b"outside 1 .. 4096" in lib.bds_last_error(ctx._h)
    assert call(cs, x, x.size, 0, k, 1.5, max_prn=13) == -1 and b"the list reaches 14" in lib.bds_last_error(ctx._h)  # PRNs 9 and 14
    # shift_b2a with carrFreqBasis 6000 instead of 6001: rint(3 spc 2000 / 6000) = spc, a whole code period
    s, x, k = dc.shift_b2a()
    x = np.array(x)
    spc = dc.sizes(s)[0]
    assert np.abs(dc.shifts(s.copy(carrFreqBasis=6000.0), k)).max() == spc
    assert call(native.pack_settings(s.copy(carrFreqBasis=6000.0)), x, x.size, 0, k, 1.5) == -1 and b"drifts" in lib.bds_last_error(ctx._h)
