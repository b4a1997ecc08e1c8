"""GPU parity: HIP acquisition (through the C ABI) vs the float64 oracle on the same int8 block.

Tolerances: codePhase exact, carrFreq exact (a grid value),
peakMetric <= 1e-6 relative.  The search grid is a sieve: every lag within kDelta of a PRN's maximum is
re-evaluated in f64 (bds_acq.hip), which is complete when the sieve errs by less than kDelta / 2 -- so the
grid is held to HALF the tolerance of its mode (GRID_TOL), not to the tolerance itself.
"""
import numpy as np
import pytest

import bds_amd
from oracle import acquisition as oacq

from helpers import (as_complex, cfg1_b2a, cfg1_b2a_iq, medium_b2a, resample_b1c, resample_b2a, small_b1c,
                     small_b1c_iq)

pytestmark = pytest.mark.gpu

# per timing()["half_storage"]: 0 fp32 storage (kDelta / 2 = 1e-5), 1 fp16 storage + fp32 arithmetic (the default; kDelta / 2 = 2e-3 since
# round 4 -- these noise-like test blocks are still held to the 1e-3 of round 3)
GRID_TOL = {0: 1e-5, 1: 1e-3}


def _compare(s, x, ctx, oracle_fn):
    diag = {}
    ref = oracle_fn(x.astype(np.complex128 if np.iscomplexobj(x) else np.float64), s, diag)
    got = bds_amd.acquisition(x, s)
    sats = [int(p) for p in s.acqSatelliteList]
    np.testing.assert_array_equal(got.codePhase, ref.codePhase)
    np.testing.assert_array_equal(got.carrFreq, ref.carrFreq)
    np.testing.assert_allclose(got.peakMetric, ref.peakMetric, rtol=1e-6, atol=0)
    nb = len(oacq.freq_bins(s))
    rm, ra = ctx.acq_grid(len(sats), nb)
    pk, dn, fb = ctx.acq_peaks(max(sats))
    for i, p in enumerate(sats):
        # the search grid is a sieve: fp32 storage ~1e-7, fp16 storage ~3e-4 of the output RMS
        np.testing.assert_allclose(rm[i], diag[p]["row_max"], rtol=GRID_TOL[ctx.timing()["half_storage"]])
        assert np.mean(ra[i] == diag[p]["row_arg"]) > (0.3 if ctx.timing()["half_storage"] else 0.9)
        assert fb[p - 1] == diag[p]["fbin"]
        np.testing.assert_allclose(pk[p - 1], diag[p]["peak"], rtol=1e-9)
    return ref, got


def test_cfg1_b2a_one_prn_three_bins(ctx):
    s, x, _ = cfg1_b2a()
    ref, got = _compare(s, x, ctx, oacq.acquisition_b2a)
    assert got.carrFreq[18] != 0  # PRN 19 detected


def test_b2a_four_prns_full_grid(ctx):
    s, x, sats = medium_b2a()
    ref, got = _compare(s, x, ctx, oacq.acquisition_b2a)
    for sat in sats:
        assert got.carrFreq[sat.prn - 1] != 0
        assert abs(got.carrFreq[sat.prn - 1] - (s.IF + sat.doppler)) <= 25


def test_b1c_reduced_rate(ctx):
    s, x, sats = small_b1c()
    ref, got = _compare(s, x, ctx, oacq.acquisition_b1c)
    assert got.carrFreq[2] != 0 and got.carrFreq[6] == 0


def test_b1c_data_only_and_short_coherent(ctx):
    s, x, _ = small_b1c(prns=(3, 7), band=300)
    s = s.copy(pilotACQflag=0, acqCohT=5, acqStep=100)
    _compare(s, x, ctx, oacq.acquisition_b1c)


def test_b2a_complex_iq_record(ctx):
    """fileType 2: longSignal = I + 1i*Q (B2a/postProcessing.m:92-96)."""
    s, x, sats = cfg1_b2a_iq()
    ref, got = _compare(s, as_complex(x), ctx, oacq.acquisition_b2a)
    assert got.carrFreq[18] != 0 and got.carrFreq[19] != 0 and got.carrFreq[20] == 0
    for sat in sats:
        assert abs(got.carrFreq[sat.prn - 1] - (s.IF + sat.doppler)) <= 25


def test_b1c_complex_iq_record(ctx):
    s, x, _ = small_b1c_iq()
    ref, got = _compare(s, as_complex(x), ctx, oacq.acquisition_b1c)
    assert got.carrFreq[2] != 0 and got.carrFreq[6] == 0


def test_b2a_resampling_branch(ctx):
    """resamplingflag = 1: fir1(700) + filtfilt + band-pass-sampling decimation before the search,
    codePhase / carrFreq mapped back afterwards (B2a/acquisition.m:54-124, 339-356)."""
    s, x, sats = resample_b2a()
    ref = oacq.acquisition_b2a(x.astype(np.float64), s)
    got = bds_amd.acquisition(x, s)
    np.testing.assert_array_equal(got.codePhase, ref.codePhase)
    np.testing.assert_array_equal(got.carrFreq, ref.carrFreq)
    np.testing.assert_allclose(got.peakMetric, ref.peakMetric, rtol=1e-6, atol=0)
    for sat in sats:
        assert abs(got.carrFreq[sat.prn - 1] - (s.IF + sat.doppler)) <= 25
        assert abs(got.codePhase[sat.prn - 1] - 1 - sat.delay) <= 4  # 48 MS/s grid mapped back to 99 MS/s
    assert got.carrFreq[20] == 0


@pytest.mark.parametrize("iq", [False, True])
def test_b1c_resampling_branch(ctx, iq):
    s, x, sats = resample_b1c(iq)
    xo = as_complex(x) if iq else x.astype(np.float64)
    ref = oacq.acquisition_b1c(xo, s)
    got = bds_amd.acquisition(xo if iq else x, s)
    np.testing.assert_array_equal(got.codePhase, ref.codePhase)
    np.testing.assert_array_equal(got.carrFreq, ref.carrFreq)
    np.testing.assert_allclose(got.peakMetric, ref.peakMetric, rtol=1e-6, atol=0)
    assert got.carrFreq[2] != 0 and got.carrFreq[11] != 0 and got.carrFreq[6] == 0


def test_fp16_overflow_fallback_reruns_in_fp32(ctx, monkeypatch):
    """A non-finite value in the fp16 search grid makes bds_acq_run repeat the whole search with fp32
    storage (forced here through the library's test hook); same acqResults, and the resampled
    settings survive the re-run."""
    for s, x, fn in ((cfg1_b2a()[0], cfg1_b2a()[1], oacq.acquisition_b2a),
                     (resample_b1c()[0], resample_b1c()[1], oacq.acquisition_b1c)):
        ref = fn(x.astype(np.float64), s)
        monkeypatch.setenv("BDS_ACQ_TEST_FORCE_FALLBACK", "1")
        ctx.reload_tuning()  # the knobs are read once per context
        try:
            got = bds_amd.acquisition(x, s, verbose=False)
            assert ctx.timing()["half_storage"] == 0
        finally:
            monkeypatch.delenv("BDS_ACQ_TEST_FORCE_FALLBACK")
            ctx.reload_tuning()
        np.testing.assert_array_equal(got.codePhase, ref.codePhase)
        np.testing.assert_array_equal(got.carrFreq, ref.carrFreq)
        np.testing.assert_allclose(got.peakMetric, ref.peakMetric, rtol=1e-6, atol=0)
        # a different configuration re-enables fp16 storage
        bds_amd.acquisition(*small_b1c()[1::-1], verbose=False)
        assert ctx.timing()["half_storage"] == 1


def test_prn_shards_sum_to_the_full_result(ctx):
    s, x, _ = medium_b2a()
    full = bds_amd.acquisition(x, s, verbose=False)
    a = bds_amd.acquisition(x, s, prn_list=[5, 19], verbose=False)
    b = bds_amd.acquisition(x, s, prn_list=[9, 33], verbose=False)
    for f in ("carrFreq", "codePhase", "peakMetric"):
        np.testing.assert_array_equal(getattr(a, f) + getattr(b, f), getattr(full, f))


def test_fp32_storage_and_generic_kernels_agree(ctx, monkeypatch):
    """The default path (fp32 arithmetic on fp16 storage; tile column pass on this 256-point plan), fp32 storage, the
    wave-private column pass forced onto the 256-point plan, the run-time generic kernels and the launch-structure variants
    (4-column tiles, plain per-PRN groups) must return the same acqResults (the f64 refinement decides in all of them)."""
    s, x, _ = medium_b2a()
    base = bds_amd.acquisition(x, s, verbose=False)
    for env in ({"BDS_ACQ_WCOLS": "1"}, {"BDS_ACQ_WCOLS": "1", "BDS_ACQ_FP16": "0"}, {"BDS_ACQ_WCOLS": "0"},
                {"BDS_ACQ_FP16": "0"}, {"BDS_ACQ_GENERIC": "1"}, {"BDS_ACQ_GENERIC_FWD": "1"},
                {"BDS_ACQ_LOGT": "2"}, {"BDS_ACQ_NOMULTI": "1"}, {"BDS_ACQ_NOMULTI": "1", "BDS_ACQ_WCOLS": "1", "BDS_ACQ_WCOLS_QCHUNK": "1"},
                {"BDS_ACQ_NOMULTI": "1", "BDS_ACQ_FP16": "0"}, {"BDS_ACQ_NOMULTI": "1", "BDS_ACQ_GROUP": "5", "BDS_ACQ_GCHUNK": "2"},
                {"BDS_ACQ_NOMULTI": "1", "BDS_ACQ_WCOLS": "1", "BDS_ACQ_GROUP": "5", "BDS_ACQ_GCHUNK": "2"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        c2 = bds_amd.native.Context(0)
        try:
            c2.acq_load(s, x)
            c2.acq_prepare(s)
            carr, cph, pm, det = c2.acq_run(s)
        finally:
            c2.close()
        for k in env:
            monkeypatch.delenv(k)
        np.testing.assert_array_equal(carr, base.carrFreq)
        np.testing.assert_array_equal(cph, base.codePhase)
        np.testing.assert_allclose(pm, base.peakMetric, rtol=1e-9)


def test_degenerate_grids_and_lists(ctx):
    """One Doppler bin (acqSearchBand = 0), an unsorted satellite list with a repeated PRN, a single PRN."""
    s, x, _ = cfg1_b2a()
    for kw in (dict(acqSearchBand=0, acqSatelliteList=[19, 20]),
               dict(acqSatelliteList=[20, 19, 19, 5]),
               dict(acqSatelliteList=[63])):
        sk = s.copy(**kw)
        ref = oacq.acquisition_b2a(x.astype(np.float64), sk)
        got = bds_amd.acquisition(x, sk, verbose=False)
        np.testing.assert_array_equal(got.codePhase, ref.codePhase)
        np.testing.assert_array_equal(got.carrFreq, ref.carrFreq)
        np.testing.assert_allclose(got.peakMetric, ref.peakMetric, rtol=1e-6, atol=0)


@pytest.mark.parametrize("l1", [256, 512, 768, 1024])
def test_every_specialised_plan_pair(ctx, monkeypatch, l1):
    """Each compile-time column length with each row length (forced factorisation), both signals: the
    search kernels of all 16 plan pairs against the oracle.  The sampling rate differs per case so that
    the context re-plans."""
    for k, l2 in enumerate((1280, 2048, 3072, 4096)):
        monkeypatch.setenv("BDS_ACQ_FORCE_L1L2", f"{l1}x{l2}")
        ctx.reload_tuning()
        fs = 10.0e6 + 1000.0 * (l1 + k)
        if k % 2 == 0:
            s = bds_amd.init_settings_b2a(samplingFreq=fs, IF=2.5e6, acqSatelliteList=[7, 19, 33], acqSearchBand=600,
                                          acqStep=200, fineNoncoh=4)
            fn, n_codes = oacq.acquisition_b2a, 7
        else:
            s = bds_amd.init_settings_b1c(samplingFreq=fs, IF=2.5e6, acqSatelliteList=[7, 19, 33], acqSearchBand=200,
                                          acqStep=100)
            fn, n_codes = oacq.acquisition_b1c, 3
        from helpers import spc_of
        from bds_amd import synth
        spc = spc_of(s)
        sats = [synth.Sat(19, 130.0, 0.41 * spc, 0.7, 47.0), synth.Sat(33, -90.0, 0.83 * spc, 2.2, 45.0)]
        x = synth.make_if(s, sats, n_codes * spc, seed=500 + l1 + k)
        ref = fn(x.astype(np.float64), s)
        got = bds_amd.acquisition(x, s, verbose=False)
        tm = ctx.timing()
        assert tm["fft_len"] == l1 * l2 and tm["half_storage"] == 1
        np.testing.assert_array_equal(got.codePhase, ref.codePhase)
        np.testing.assert_array_equal(got.carrFreq, ref.carrFreq)
        np.testing.assert_allclose(got.peakMetric, ref.peakMetric, rtol=1e-6, atol=0)
        assert got.carrFreq[18] != 0
    monkeypatch.delenv("BDS_ACQ_FORCE_L1L2")
    ctx.reload_tuning()


@pytest.mark.parametrize("sig", ["b2a", "b1c"])
def test_both_row_pass_kernels_on_4096_point_rows(ctx, monkeypatch, sig):
    """4096-point rows have two row-pass kernels: the wave-private one (bds_acq_wrows.h, default) and k_rows_inv_f
    (BDS_ACQ_WROWS=0).  Both, with fp16 and fp32 storage, one component (B2a) and two (B1C), against the oracle; the coarse
    grid agrees with the oracle's between the two kernels to the sieve tolerance, the results exactly."""
    from helpers import spc_of
    from bds_amd import synth
    monkeypatch.setenv("BDS_ACQ_FORCE_L1L2", "512x4096")
    fs = 10.1e6
    if sig == "b2a":
        s = bds_amd.init_settings_b2a(samplingFreq=fs, IF=2.5e6, acqSatelliteList=[7, 19, 33], acqSearchBand=600, acqStep=200,
                                      fineNoncoh=4)
        fn, n_codes = oacq.acquisition_b2a, 7
    else:
        s = bds_amd.init_settings_b1c(samplingFreq=fs, IF=2.5e6, acqSatelliteList=[7, 19, 33], acqSearchBand=200, acqStep=100)
        fn, n_codes = oacq.acquisition_b1c, 3
    spc = spc_of(s)
    sats = [synth.Sat(19, 130.0, 0.41 * spc, 0.7, 47.0), synth.Sat(33, -90.0, 0.83 * spc, 2.2, 45.0)]
    x = synth.make_if(s, sats, n_codes * spc, seed=77)
    ref = fn(x.astype(np.float64), s)
    try:
        for env in ({}, {"BDS_ACQ_WROWS": "0"}, {"BDS_ACQ_FP16": "0"}, {"BDS_ACQ_FP16": "0", "BDS_ACQ_WROWS": "0"},
                    {"BDS_ACQ_GCHUNK": "1"}, {"BDS_ACQ_ROWS_GRID": "64"}, {"BDS_ACQ_CLOCKPROBE": "1"}):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            c2 = bds_amd.native.Context(0)
            try:
                c2.acq_load(s, x)
                c2.acq_prepare(s)
                carr, cph, pm, det = c2.acq_run(s)
                assert c2.timing()["fft_len"] == 512 * 4096
                # the clock probe (sampled workgroups time themselves: shader clock against reference clock) reports the engine
                # clock of the search kernels only when asked to
                ghz = c2.timing()["shader_clock_GHz"]
                assert (0.5 < ghz < 3.0) if "BDS_ACQ_CLOCKPROBE" in env else ghz == 0.0
            finally:
                c2.close()
            for k in env:
                monkeypatch.delenv(k)
            np.testing.assert_array_equal(cph, ref.codePhase, err_msg=str(env))
            np.testing.assert_array_equal(carr, ref.carrFreq, err_msg=str(env))
            np.testing.assert_allclose(pm, ref.peakMetric, rtol=1e-6, atol=0, err_msg=str(env))
            assert carr[18] != 0
    finally:
        monkeypatch.delenv("BDS_ACQ_FORCE_L1L2")
        ctx.reload_tuning()


# environment -> (rows_kernel, cols_kernel, kernel_flags) of bds_timing on the forced 768 x 4096 plan, B1C with both components
KERNELS_768x4096 = [
    ({}, (2, 2, 3)),
    ({"BDS_ACQ_NOMULTI": "1"}, (2, 2, 3)),  # (one PRN's cells per launch pair, no cell list)
    ({"BDS_ACQ_PK": "0"}, (2, 2, 1)),
    ({"BDS_ACQ_PK": "2"}, (2, 2, 3)),       # (packed butterflies in the row pass only: the flag is the row pass's)
    ({"BDS_ACQ_ILV": "0"}, (2, 2, 2)),
    ({"BDS_ACQ_PK": "0", "BDS_ACQ_ILV": "0"}, (2, 2, 0)),
    ({"BDS_ACQ_WROWS": "0"}, (1, 2, 0)),
    ({"BDS_ACQ_WCOLS": "0"}, (2, 1, 2)),
    ({"BDS_ACQ_FP16": "0"}, (1, 2, 0)),
]


def test_reported_kernels_on_the_768x4096_plan(ctx, monkeypatch):
    """The wave-private pair of the 768 x 4096 plan has an interleaved and a packed variant of each pass, chosen by the tuning knobs;
    at a small grid (3 PRNs x 5 bins on a forced plan) every choice runs against the oracle, and the timing record names the kernels
    and variants that ran.  The last row is B2a on the same plan: its two components (data and pilot) are interleaved like B1C's."""
    from helpers import spc_of
    from bds_amd import synth
    monkeypatch.setenv("BDS_ACQ_FORCE_L1L2", "768x4096")
    fs = 10.1e6
    s1 = bds_amd.init_settings_b1c(samplingFreq=fs, IF=2.5e6, acqSatelliteList=[7, 19, 33], acqSearchBand=200, acqStep=100)
    s2 = bds_amd.init_settings_b2a(samplingFreq=fs, IF=2.5e6, acqSatelliteList=[7, 19, 33], acqSearchBand=600, acqStep=200,
                                   fineNoncoh=4)
    cases = {}
    for name, s, fn, n_codes in (("b1c", s1, oacq.acquisition_b1c, 3), ("b2a", s2, oacq.acquisition_b2a, 7)):
        spc = spc_of(s)
        sats = [synth.Sat(19, 130.0, 0.41 * spc, 0.7, 47.0), synth.Sat(33, -90.0, 0.83 * spc, 2.2, 45.0)]
        x = synth.make_if(s, sats, n_codes * spc, seed=77)
        cases[name] = (s, x, fn(x.astype(np.float64), s))
    try:
        for sig, env, want in [("b1c", e, w) for e, w in KERNELS_768x4096] + [("b2a", {}, (2, 2, 3))]:
            s, x, ref = cases[sig]
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            c2 = bds_amd.native.Context(0)
            try:
                c2.acq_load(s, x)
                c2.acq_prepare(s)
                carr, cph, pm, det = c2.acq_run(s)
                tm = c2.timing()
            finally:
                c2.close()
            for k in env:
                monkeypatch.delenv(k)
            what = f"{sig} {env}"
            print(what, int(tm["fft_len"]), (int(tm["rows_kernel"]), int(tm["cols_kernel"]), int(tm["kernel_flags"])))
            assert tm["fft_len"] == 768 * 4096, what
            np.testing.assert_array_equal(cph, ref.codePhase, err_msg=what)
            np.testing.assert_array_equal(carr, ref.carrFreq, err_msg=what)
            np.testing.assert_allclose(pm, ref.peakMetric, rtol=1e-6, atol=0, err_msg=what)
            assert (tm["rows_kernel"], tm["cols_kernel"], tm["kernel_flags"]) == want, what
    finally:
        monkeypatch.delenv("BDS_ACQ_FORCE_L1L2")
        ctx.reload_tuning()


def test_data_type_other_than_schar_is_rejected(ctx):
    """settings.dataType (fread(fid, ..., settings.dataType), B2a/tracking.m:237-238): only int8 records."""
    s, x, _ = cfg1_b2a()
    with pytest.raises(bds_amd.native.BdsError, match="dataType"):
        bds_amd.acquisition(x, s.copy(dataType="int16"), verbose=False)


def test_b1c_guard_moves_a_late_twin_peak_back(ctx):
    """B1C/acquisition.m:239-241: the 20-ms circular correlation has twin peaks one code period apart; when the
    maximum is the LATE twin and its code period would run past the end of longSignal, codePhase is moved back by
    samplesPerCode.  longSignal of 2*spc + 20 samples, seed chosen (with the oracle) so that the late twin wins."""
    from bds_amd import synth
    from helpers import spc_of

    s = bds_amd.init_settings_b1c(samplingFreq=5e6, IF=1.2e6, acqSatelliteList=[7], acqSearchBand=100, acqStep=50)
    spc = spc_of(s)
    x = synth.make_if(s, [synth.Sat(7, 40.0, 0.55 * spc, 1.0, 47.0)], 2 * spc + 20, seed=3)
    ref = oacq.acquisition_b1c(x.astype(np.float64), s)
    got = bds_amd.acquisition(x, s, verbose=False)
    assert ref.codePhase[6] == 27502  # the early twin's position ...
    lags = ctx.acq_candidates(7)[:, 1]
    assert 27502 + spc in lags  # ... although the search maximum sits one code period later: the guard fired
    np.testing.assert_array_equal(got.codePhase, ref.codePhase)
    np.testing.assert_array_equal(got.carrFreq, ref.carrFreq)
    np.testing.assert_allclose(got.peakMetric, ref.peakMetric, rtol=1e-6)


def test_fine_search_carrier_of_exactly_zero_becomes_one(ctx):
    """acquisition.m:303-305 (B2a :333-335): carrFreq == 0 would read as "not detected", so it is stored as 1."""
    from bds_amd import synth
    from helpers import spc_of

    s = bds_amd.init_settings_b1c(samplingFreq=5e6, IF=25.0, acqSatelliteList=[7], acqSearchBand=100, acqStep=50)
    spc = spc_of(s)
    x = synth.make_if(s, [synth.Sat(7, -25.0, 0.3 * spc, 0.4, 50.0)], 3 * spc, seed=4)  # carrier at 0 Hz
    ref = oacq.acquisition_b1c(x.astype(np.float64), s)
    got = bds_amd.acquisition(x, s, verbose=False)
    assert ref.carrFreq[6] == 1.0 and got.carrFreq[6] == 1.0
    np.testing.assert_array_equal(got.codePhase, ref.codePhase)
    np.testing.assert_allclose(got.peakMetric, ref.peakMetric, rtol=1e-6)


def test_tuning_reload_rebuilds_the_spectrum_layout(ctx, monkeypatch):
    """The wave-private row pass reads spectrum rows in its own element order (wrows_perm, written so by the forward row pass),
    k_rows_inv_f in natural order.  Switching between them on ONE context with UNCHANGED settings must rebuild the cached code
    spectra: bds_reload_tuning invalidates the acquisition configuration."""
    from helpers import spc_of
    from bds_amd import synth
    monkeypatch.setenv("BDS_ACQ_FORCE_L1L2", "512x4096")
    ctx.reload_tuning()
    try:
        s = bds_amd.init_settings_b1c(samplingFreq=10.3e6, IF=2.5e6, acqSatelliteList=[7, 19, 33], acqSearchBand=200, acqStep=100)
        spc = spc_of(s)
        sats = [synth.Sat(19, 130.0, 0.41 * spc, 0.7, 47.0), synth.Sat(33, -90.0, 0.83 * spc, 2.2, 45.0)]
        x = synth.make_if(s, sats, 3 * spc, seed=78)
        ref = oacq.acquisition_b1c(x.astype(np.float64), s)
        for wrows, kernel in (("1", 2), ("0", 1), ("1", 2)):
            monkeypatch.setenv("BDS_ACQ_WROWS", wrows)
            ctx.reload_tuning()
            got = bds_amd.acquisition(x, s, verbose=False)
            tm = ctx.timing()
            assert tm["rows_kernel"] == kernel and tm["half_storage"] == 1, (wrows, tm)
            np.testing.assert_array_equal(got.codePhase, ref.codePhase, err_msg=wrows)
            np.testing.assert_array_equal(got.carrFreq, ref.carrFreq, err_msg=wrows)
            np.testing.assert_allclose(got.peakMetric, ref.peakMetric, rtol=1e-6, atol=0, err_msg=wrows)
    finally:
        monkeypatch.delenv("BDS_ACQ_FORCE_L1L2", raising=False)
        monkeypatch.delenv("BDS_ACQ_WROWS", raising=False)
        ctx.reload_tuning()


@pytest.mark.parametrize("case", ["b2a", "b2a_iq", "b1c", "b1c_iq", "b1c_data_only"])
def test_device_refinement_chain_equals_the_host_path(case, monkeypatch):
    """Round 5: candidates -> f64 sums -> peak -> (B2a) second peak -> threshold -> fine search as one chain of launches with a
    single download (csrc/bds_acq_refine.h), against the host-driven refinement of rounds 1-4 (BDS_ACQ_HOSTREFINE=1): the same
    acqResults, f64 peaks, normalisers, winning bins and refined candidate cells, bit for bit -- real and I/Q records, one
    and two components."""
    cplx = case.endswith("_iq")
    if case == "b2a":
        s, x, _ = medium_b2a()
        prns = [5, 9, 19, 33]
    elif case == "b2a_iq":
        s, x, _ = cfg1_b2a_iq()
        prns = [int(p) for p in s.acqSatelliteList]
    elif case == "b1c_iq":
        s, x, _ = small_b1c_iq()
        prns = [int(p) for p in s.acqSatelliteList]
    else:
        s, x, _ = small_b1c()
        prns = [3, 7, 12]
        if case == "b1c_data_only":
            s = s.copy(pilotACQflag=0)
    monkeypatch.setenv("BDS_VERBOSE", "1")  # a hand-over to the host path names its reason on stderr (shown when the test fails)
    if case.startswith("b1c"):
        # (these reduced-rate blocks plan 256 x 2048, where the tile column pass with its per-tile records is the default and
        #  the host path its refinement: the wave-private pass -- what cfg3 runs -- is switched on for them)
        monkeypatch.setenv("BDS_ACQ_WCOLS", "1")
    out = {}
    for host in ("0", "1"):
        if host == "1":
            monkeypatch.setenv("BDS_ACQ_HOSTREFINE", "1")
        c = bds_amd.native.Context(0)
        try:
            c.acq_load(s, x, is_complex=cplx)
            c.acq_prepare(s)
            res = c.acq_run(s)
            tm = c.timing()
            out[host] = (res, c.acq_peaks(63), [c.acq_candidates(p) for p in prns])
        finally:
            c.close()
        assert tm["refine_path"] == (1 if host == "0" else 0), tm
    for u, v in zip(out["0"][0], out["1"][0]):
        assert np.array_equal(u, v)
    assert np.count_nonzero(out["0"][0][0]) >= 1
    for u, v in zip(out["0"][1], out["1"][1]):
        assert np.array_equal(u, v)
    for u, v in zip(out["0"][2], out["1"][2]):
        assert len(u) > 0 and np.array_equal(u, v)


def test_device_chain_hands_over_when_the_band_holds_more_candidates_than_it_keeps(monkeypatch):
    """The device chain keeps 16 384 candidates per stage.  With the tolerance forced to 40 % the two absent PRNs of this block
    alone put ~40 000 cells into the band (a noise surface of 5e6 Rayleigh cells: exp(-5.5) of them exceed 0.6 of the maximum):
    the chain must flag the overflow and hand the run to the host path (refine_path 0), whose results equal the default run's."""
    s, x, _ = medium_b2a()
    base = bds_amd.acquisition(x, s, verbose=False)
    monkeypatch.setenv("BDS_ACQ_KDELTA", "0.4")
    monkeypatch.setenv("BDS_VERBOSE", "1")
    c = bds_amd.native.Context(0)
    try:
        c.acq_load(s, x)
        c.acq_prepare(s)
        carr, cph, pm, _ = c.acq_run(s)
        tm = c.timing()
        ncand = sum(len(c.acq_candidates(p)) for p in (5, 9, 19, 33))
    finally:
        c.close()
    assert ncand > 16384, ncand
    assert tm["refine_path"] == 0, tm
    np.testing.assert_array_equal(carr, base.carrFreq)
    np.testing.assert_array_equal(cph, base.codePhase)
    np.testing.assert_allclose(pm, base.peakMetric, rtol=1e-12)


def test_b2a_above_the_rate_the_register_column_pass_covers(ctx):
    """the 80 x 4096 plan's register column pass forms output rows 0 .. 48 only, i.e. lags below 200 704 --
    enough for N = 198 750 at 99.375 MS/s, not for N = 210 000 at 105 MS/s, where its cost bonus used to pick it all the same and
    lags >= 200 704 were silently never searched.  Here a satellite sits at 0.97 of a code period, so that its second-period
    peak (lag ~ 206 850) lies beyond row 48: the plan must be another one and the results the oracle's."""
    from helpers import spc_of
    from bds_amd import synth
    s = bds_amd.init_settings_b2a(samplingFreq=105.0e6, IF=14.58e6, acqSatelliteList=[19, 20, 21], acqSearchBand=800, acqStep=400,
                                  fineNoncoh=3)
    spc = spc_of(s)
    assert 2 * spc == 210000
    sats = [synth.Sat(19, 310.0, 0.97 * spc, 1.1, 47.0), synth.Sat(20, -200.0, 0.31 * spc, 0.3, 46.0)]
    x = synth.make_if(s, sats, 6 * spc, seed=4105)
    ref, got = _compare(s, x, ctx, oacq.acquisition_b2a)
    tm = ctx.timing()
    assert tm["plan_l1"] != 80 and tm["n_circ"] == 210000, tm
    assert got.carrFreq[18] != 0 and got.carrFreq[19] != 0
    # and the plan is still the small one where it does cover every lag (cfg2's rate)
    s2, x2, _ = cfg1_b2a()
    bds_amd.acquisition(x2, s2, verbose=False)
    assert ctx.timing()["plan_l1"] == 80
