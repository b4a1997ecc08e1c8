"""The opt-in N-point search pair for B1C at 30.69 MS/s (csrc/bds_acq_pfa31.h: N = 613 800 = 31 x 11 x 1800, bds_acq_set_b1c_npoint): which
settings take it with the switch on, that it reports and decides what the float64 oracle decides, and that acqResults, the f64 peaks and
the detected flags are the same BITS as the same settings give with the switch off (the zero-padded L-point pair).  Candidate lists are
not compared: the two sieves differ.  N is fixed by the feature, so the small shapes are the PRN list and the Doppler band."""
import os

import numpy as np
import pytest

import bds_amd
from bds_amd import synth
from oracle import acquisition as oacq

pytestmark = pytest.mark.gpu
N = 613800
K1, K2, K3 = 31, 11, 1800
TILE, WAVE = 16, 4
SPC = 306900
FS, IF = 30.69e6, 7.5e6
LOBE = 0  # a synthetic satellite whose code period starts at sample d has the sieve's maximum at the 0-based lag d + LOBE at this rate


def lag_of(t1, t2, t3):
    return (t1 * (N // K1) + t2 * (N // K2) + t3 * (N // K3)) % N


def coords(lag):
    """(t1, t2, t3) with lag_of(t1, t2, t3) == lag"""
    return tuple(lag * pow(N // k % k, -1, k) % k for k in (K1, K2, K3))


def _cpus():
    return max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 4))


def _settings(**kw):
    return bds_amd.init_settings_b1c(samplingFreq=FS, IF=IF, **kw)


def _run(monkeypatch, s, x, prns, on, env=None, is_complex=None, ctx=None):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    c = ctx or bds_amd.native.Context(0)  # the knobs are read once, at context creation
    for k in (env or {}):
        monkeypatch.delenv(k)
    try:
        c.acq_set_b1c_npoint(on)
        if is_complex is None:
            c.acq_load(s, x)
        else:
            c.acq_load(s, x, is_complex)
        c.acq_prepare(s)
        res = c.acq_run(s, prn_list=prns)
        tm = c.timing()
        grid, arg = c.acq_grid(len(prns), int(tm["n_bins"]))
        pk, dn, fb = c.acq_peaks(63)
    finally:
        if ctx is None:
            c.close()
    return res, tm, grid.copy(), arg.copy(), pk, dn, fb


def _same_bits(a, b):
    for u, v in zip(a[0], b[0]):
        assert np.array_equal(u, v)              # carrFreq, codePhase, peakMetric, detected
    np.testing.assert_array_equal(a[4], b[4])    # f64 peaks
    np.testing.assert_array_equal(a[6], b[6])    # winning bins
    np.testing.assert_allclose(a[2], b[2], rtol=2e-3)  # the two sieves' cell maxima: within kDelta / 2 of each other


def _on_the_pair(tm):
    return (tm["rows_kernel"], tm["cols_kernel"], tm["fft_len"], tm["plan_l1"], tm["plan_l2"]) == (3, 4, N, K1 * K2, K3)


def _on_l_point(tm):
    return tm["rows_kernel"] in (1, 2) and tm["fft_len"] > N


# Satellites whose correlation peaks sit at the first / last index of the 31- and 11-point dimensions and, in the 1800-point rows, at
# lag 0 and 1799, on both sides of a wave's 4 lags (3 | 4), of a tile of the inter-pass buffer (15 | 16) and of the short last tile
# (1791 | 1792).  The 20 ms hold two code periods: the peak one period on has the same (t1, t2) and t3 + 900 (N / 2 = 4 x N / 8).
EDGES = [(0, 0, 0), (30, 10, 1799), (15, 5, 15), (1, 6, 16), (29, 4, 1791), (7, 1, 1792), (20, 9, 3), (11, 2, 4)]
PRNS = [3, 11, 17, 29, 41, 53, 8, 22]
BINS = [0, 20, 1, 19, 10, 7, 13, 4]  # the first and the last bin of the 21
ABSENT = 5


@pytest.fixture(scope="module")
def block():
    s = _settings(acqSatelliteList=sorted(PRNS + [ABSENT]), acqSearchBand=500.0)
    assert (s.acqCohT, s.acqStep, s.pilotACQflag) == (10, 50, 1)
    lags = [lag_of(*e) for e in EDGES]
    sats = [synth.Sat(p, -500.0 + 50.0 * b, float((t - LOBE) % SPC), 0.3 + i, 50.0) for i, (p, b, t) in enumerate(zip(PRNS, BINS, lags))]
    return s, synth.make_if(s, sats, 4 * SPC, seed=31, code_doppler=False), lags


def test_switch_on_against_the_oracle_and_against_switch_off(block, monkeypatch):
    from oracle import cfast

    cfast.build()
    s, x, lags = block
    prns = list(s.acqSatelliteList)
    a = _run(monkeypatch, s, x, prns, True)
    b = _run(monkeypatch, s, x, prns, False)
    assert (a[1]["rows_kernel"], a[1]["cols_kernel"], a[1]["fft_len"]) == (3, 4, 613800)
    assert _on_the_pair(a[1]) and a[1]["n_bins"] == 21 and a[1]["half_storage"] == 1
    assert _on_l_point(b[1])
    _same_bits(a, b)
    ref = oacq.acquisition_b1c(x.astype(np.float64), s, coarse=cfast.backend(threads=_cpus()))
    for r in (a, b):
        np.testing.assert_array_equal(r[0][1], ref.codePhase)
        np.testing.assert_array_equal(r[0][0], ref.carrFreq)
        np.testing.assert_allclose(r[0][2], ref.peakMetric, rtol=1e-6)
    assert a[0][0][ABSENT - 1] == 0
    seen = []
    for i, (p, bin_, e) in enumerate(zip(PRNS, BINS, EDGES)):
        assert a[0][0][p - 1] != 0, p
        assert int(a[6][p - 1]) == bin_ + 1, (p, int(a[6][p - 1]), bin_)
        lag = int(a[3][prns.index(p)][bin_])  # the sieve's maximum of the winning cell, 1-based
        assert lag == int(b[3][prns.index(p)][bin_]), p
        t1, t2, t3 = coords(lag - 1)
        assert (t1, t2) == e[:2] and t3 in (e[2], (e[2] + 900) % K3), (p, e, (t1, t2, t3))
        seen.append((t1, t2, t3))
    assert {t[0] for t in seen} >= {0, K1 - 1} and {t[1] for t in seen} >= {0, K2 - 1}


def test_doppler_steps_of_two_bins(block, monkeypatch):
    """acqStep = 100 Hz is two spectrum bins per Doppler bin (acqStep N / fs = 2)"""
    s0, x, _ = block
    s = s0.copy(acqStep=100.0, acqSearchBand=500.0)
    prns = [3, 5, 11]
    a = _run(monkeypatch, s, x, prns, True)
    b = _run(monkeypatch, s, x, prns, False)
    assert _on_the_pair(a[1]) and a[1]["n_bins"] == 11 and _on_l_point(b[1])
    _same_bits(a, b)
    assert a[0][0][3 - 1] != 0 and a[0][0][11 - 1] != 0 and a[0][0][5 - 1] == 0


def test_iq_record(monkeypatch):
    """fileType 2 (interleaved I/Q int8, B1C/postProcessing.m:92-96): the complex block through the N-point pair"""
    from bds_amd.acquisition import _as_int8
    from helpers import as_complex

    s = _settings(acqSatelliteList=list(range(1, 64)), fileType=2, acqSearchBand=250.0)
    sats = [synth.Sat(7, -230.0, 0.613 * SPC, 0.7, 45.0), synth.Sat(23, 210.0, 0.2 * SPC, 2.0, 46.0)]
    x, is_complex = _as_int8(as_complex(synth.make_if(s, sats, 4 * SPC, seed=77, iq_sign=-1)), s)
    assert is_complex
    prns = [7, 8, 23]
    a = _run(monkeypatch, s, x, prns, True, is_complex=True)
    b = _run(monkeypatch, s, x, prns, False, is_complex=True)
    assert _on_the_pair(a[1]) and a[1]["n_bins"] == 11 and _on_l_point(b[1])
    _same_bits(a, b)
    assert a[0][0][6] != 0 and a[0][0][22] != 0 and a[0][0][7] == 0
    assert abs(a[0][0][6] - (s.IF - 230.0)) <= 25


def test_acquisition_keyword_and_a_part_of_the_prn_list(block):
    """bds_amd.acquisition(..., b1c_npoint=True) sets the process-wide context's switch; a shard of the PRN list runs on the pair too"""
    s, x, _ = block
    try:
        on = bds_amd.acquisition(x, s, prn_list=[3, 5], verbose=False, b1c_npoint=True)
        assert _on_the_pair(bds_amd.get_context(0).timing())
        off = bds_amd.acquisition(x, s, prn_list=[3, 5], verbose=False, b1c_npoint=False)
        assert _on_l_point(bds_amd.get_context(0).timing())
    finally:
        bds_amd.get_context(0).acq_set_b1c_npoint(False)
    for f in ("carrFreq", "codePhase", "peakMetric"):
        np.testing.assert_array_equal(getattr(on, f), getattr(off, f))
    assert on.carrFreq[3 - 1] != 0 and on.carrFreq[5 - 1] == 0


def test_the_switch_is_off_by_default(block, monkeypatch):
    s, x, _ = block
    c = bds_amd.native.Context(0)
    try:
        c.acq_load(s, x)
        c.acq_prepare(s)
        c.acq_run(s, prn_list=[3])
        assert _on_l_point(c.timing())
    finally:
        c.close()


@pytest.mark.parametrize("change,env,int16,why", [
    (dict(pilotACQflag=0), None, False, "one component"),
    (dict(acqStep=25.0, acqSearchBand=250.0), None, False, "half a spectrum bin per Doppler step"),
    (dict(acqCohT=5), None, False, "N = 10 ms of samples"),
    (dict(resamplingflag=1, resamplingThreshold=20e6), None, False, "the search runs on the resampled block"),
    (dict(dataType="int16"), None, True, "an int16 block"),
    (dict(), {"BDS_ACQ_PFA": "0"}, False, "the N-point pairs are switched off"),
    (dict(), {"BDS_ACQ_FP16": "0"}, False, "fp32 storage"),
])
def test_settings_the_pair_does_not_cover_take_the_l_point_pair_with_the_switch_on(monkeypatch, change, env, int16, why):
    s = _settings(acqSearchBand=250.0).copy(**change)
    spc = int(round(s.samplingFreq * 10e-3))
    x = synth.make_if(s.copy(dataType="schar") if int16 else s, [synth.Sat(19, -208.0, 0.613 * spc, 0.7, 47.0)], 4 * spc, seed=53)
    if int16:
        x = x.astype(np.int16) * 256
    res, tm, *_ = _run(monkeypatch, s, x, [19, 20], True, env)
    assert res[0][19 - 1] != 0 and res[0][20 - 1] == 0
    assert tm["rows_kernel"] in (0, 1, 2) and tm["cols_kernel"] != 4 and tm["fft_len"] != N, why


@pytest.mark.parametrize("fs,n,l1,l2", [(53e6, 1060000, 53 * 32, 625), (99.375e6, 1987500, 53 * 12, 3125)])
def test_the_other_rates_keep_their_own_pairs_with_the_switch_on(monkeypatch, fs, n, l1, l2):
    s = bds_amd.init_settings_b1c(samplingFreq=fs, acqSearchBand=100.0)
    spc = int(round(fs * 10e-3))
    x = synth.make_if(s, [synth.Sat(19, -58.0, 0.613 * spc, 0.7, 47.0)], 4 * spc, seed=53)
    res, tm, *_ = _run(monkeypatch, s, x, [19, 20], True)
    assert res[0][19 - 1] != 0 and res[0][20 - 1] == 0
    assert (tm["rows_kernel"], tm["cols_kernel"], tm["fft_len"], tm["plan_l1"], tm["plan_l2"]) == (3, 4, n, l1, l2)


def test_all_zero_block_falls_back_and_the_next_block_is_served_again(block):
    """an all-zero block is one exact tie over every lag: the candidate list runs over and the call is redone on the L-point pair with fp32
    storage, then on the run-time-plan kernels: nothing detected, and the next block on the same context starts on the N-point pair again"""
    s0, x, _ = block
    s = s0.copy(acqSearchBand=100.0)
    c = bds_amd.native.Context(0)
    try:
        c.acq_set_b1c_npoint(True)
        c.acq_load(s, np.zeros(len(x), dtype=np.int8))
        c.acq_prepare(s)
        res = c.acq_run(s, prn_list=[3, 5])
        assert not np.any(res[0]) and not np.any(res[1])
        assert c.timing()["fft_len"] != N
        c.acq_load(s, x)
        c.acq_prepare(s)
        res = c.acq_run(s, prn_list=[41, 5])  # (PRN 41 sits at 0 Hz, inside the +-100 Hz band)
        assert _on_the_pair(c.timing())
        assert res[0][41 - 1] != 0 and res[0][5 - 1] == 0
    finally:
        c.close()


def test_30_69_and_53_msps_alternate_on_one_context(block, monkeypatch):
    """30.69 MS/s (bds_acq_pfa31.h), 53 MS/s (bds_acq_pfa32.h), 30.69 MS/s again on one context: the cached code spectra are dropped when the
    layout changes, each run reports its own pair, and the first and third runs agree bit for bit"""
    s31, x31, _ = block
    s31 = s31.copy(acqSearchBand=100.0)
    s53 = bds_amd.init_settings_b1c(acqSearchBand=100.0)
    spc53 = 530000
    x53 = synth.make_if(s53, [synth.Sat(19, -58.0, 0.613 * spc53, 0.7, 47.0)], 4 * spc53, seed=53)
    c = bds_amd.native.Context(0)
    out = []
    try:
        c.acq_set_b1c_npoint(True)
        for s, x, prns in ((s31, x31, [41, 5]), (s53, x53, [19, 20]), (s31, x31, [41, 5])):
            out.append(_run(monkeypatch, s, x, prns, True, ctx=c))
    finally:
        c.close()
    assert [o[1]["fft_len"] for o in out] == [N, 1060000, N]
    assert [(o[1]["rows_kernel"], o[1]["cols_kernel"]) for o in out] == [(3, 4)] * 3
    assert _on_the_pair(out[0][1]) and _on_the_pair(out[2][1]) and (out[1][1]["plan_l1"], out[1][1]["plan_l2"]) == (53 * 32, 625)
    for u, v in zip(out[0][0], out[2][0]):
        assert np.array_equal(u, v)
    np.testing.assert_array_equal(out[0][2], out[2][2])
    np.testing.assert_array_equal(out[0][3], out[2][3])
    np.testing.assert_array_equal(out[0][4], out[2][4])
    assert out[0][0][0][41 - 1] != 0 and out[0][0][0][5 - 1] == 0
    assert out[1][0][0][19 - 1] != 0 and out[1][0][0][20 - 1] == 0


def test_full_size_switch_on_against_switch_off(monkeypatch):
    """all 63 PRNs x 201 bins at 30.69 MS/s: the same bits from both pairs"""
    s = _settings(acqSatelliteList=list(range(1, 64)))
    sats = [synth.Sat(19, -1730.0, 0.613 * SPC, 0.7, 45.0), synth.Sat(35, 2210.0, 0.2 * SPC, 2.0, 46.0), synth.Sat(46, 4990.0, 0.41 * SPC, 1.1, 47.0)]
    x = synth.make_if(s, sats, 4 * SPC, seed=53)
    prns = list(s.acqSatelliteList)
    a = _run(monkeypatch, s, x, prns, True)
    b = _run(monkeypatch, s, x, prns, False)
    assert _on_the_pair(a[1]) and a[1]["n_prn"] == 63 and a[1]["n_bins"] == 201 and _on_l_point(b[1])
    _same_bits(a, b)
    assert set(np.nonzero(a[0][0])[0] + 1) == {sat.prn for sat in sats}
