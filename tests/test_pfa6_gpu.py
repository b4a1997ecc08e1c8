"""The opt-in N-point search pair for B2a at 99.375 MS/s (csrc/bds_acq_pfa6.h: N = 198 750 = 53 x 6 x 625, bds_acq_set_b2a_npoint): which
settings take it with the switch on, that it reports and decides what the float64 oracle decides, and that acqResults, the f64 peaks and
the second peaks are the same BITS as the same settings give with the switch off (the zero-padded 80 x 4096 pair).  Candidate lists are
not compared: the two sieves differ.  N is fixed by the feature, so the small shape is the PRN list."""
import os

import numpy as np
import pytest

import bds_amd
from bds_amd import synth
from oracle import acquisition as oacq

pytestmark = pytest.mark.gpu
N = 198750
K1, K2, K3 = 53, 6, 625
TILE, WAVE = 32, 8
SPC = 99375


def lag_of(t1, t2, t3):
    return (t1 * (N // K1) + t2 * (N // K2) + t3 * (N // K3)) % N


def _cpus():
    return max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 4))


def _run(monkeypatch, s, x, prns, on, env=None, is_complex=None, ctx=None):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    c = ctx or bds_amd.native.Context(0)  # the knobs are read once, at context creation
    for k in (env or {}):
        monkeypatch.delenv(k)
    try:
        c.acq_set_b2a_npoint(on)
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
    np.testing.assert_array_equal(a[5], b[5])    # f64 second peaks
    np.testing.assert_array_equal(a[6], b[6])    # winning bins
    np.testing.assert_allclose(a[2], b[2], rtol=2e-3)  # the two sieves' cell maxima: within kDelta / 2 of each other


def _on_the_pair(tm):
    return (tm["rows_kernel"], tm["cols_kernel"], tm["fft_len"], tm["plan_l1"], tm["plan_l2"]) == (3, 4, N, K1 * K2, K3)


def _on_l_point(tm):
    return tm["rows_kernel"] in (1, 2) and tm["fft_len"] != N


def coords(lag):
    """(t1, t2, t3) with lag_of(t1, t2, t3) == lag"""
    return tuple(lag * pow(N // k % k, -1, k) % k for k in (K1, K2, K3))


def delay_of(lag):
    """synth.Sat delay that puts the correlation peak on 0-based lag `lag` (mod one code period): a code period that starts at sample d
    peaks at lag d + 1 of the search, the reference's codePhase d + 2"""
    return float((lag - 1) % SPC)


# Satellites.  The winning bins b = 5 m + j cover j = 0 .. 4 at m = 0, and m = 5 (bin 25, the last).
# Two sit at the ENDS of the 2 ms: the peaks of a satellite lie one code period apart (lag and lag + spc: the same t1 and t3, t2 + 3),
# equal but for the noise, and the seed is one for which PRN 3 (delay 1) wins in the first period, codePhase 3, and PRN 11
# (delay spc - 3) in the second, codePhase N - 1 (the float64 oracle: 5.7 % and 4.0 % above the other period's peak).  The second peak
# is searched outside +-20 samples of the winner, so PRN 3 has no left range and PRN 11 no right one.
# The others are built through lag_of to sit on EDGES: the first / last t1, and t3 on both sides of a wave's 8 lags (7 | 8), of a
# tile (31 | 32), at 607 | 608 (the last full tile), at 624 (the wave of the last tile with one live lag) and at 0.
EDGES = [(0, 0, 7), (52, 5, 8), (26, 1, 31), (1, 2, 32), (51, 4, 607), (13, 3, 608), (7, 0, 624), (40, 2, 0)]
ENDS = {3: 3, 11: N - 1}  # PRN: codePhase
BINS = [0, 25, 1, 2, 3, 4, 12, 19, 7, 21]
PRNS = [3, 11, 17, 29, 41, 53, 8, 22, 35, 44]
ABSENT = 5
S2C = 20  # samples2CodeChip (B2a/acquisition.m:137) at 99.375 MS/s: ceil(fs / codeFreqBasis) * 2


@pytest.fixture(scope="module")
def block():
    s = bds_amd.init_settings_b2a(acqSatelliteList=sorted(PRNS + [ABSENT]))
    assert (s.samplingFreq, s.acqStep, s.acqSearchBand) == (99.375e6, 400, 5000)
    delays = [1.0, float(SPC - 3)] + [delay_of(lag_of(*e)) for e in EDGES]
    sats = [synth.Sat(p, -5000.0 + 400.0 * b, d, 0.3 + i, 50.0) for i, (p, b, d) in enumerate(zip(PRNS, BINS, delays))]
    x = synth.make_if(s, sats, 17 * SPC, seed=100, code_doppler=False)
    return s, x, sats, delays


def test_switch_on_against_the_oracle_and_against_switch_off(block, monkeypatch):
    from oracle import cfast

    cfast.build()
    s, x, sats, delays = block
    prns = list(s.acqSatelliteList)
    a = _run(monkeypatch, s, x, prns, True)
    b = _run(monkeypatch, s, x, prns, False)
    assert (a[1]["rows_kernel"], a[1]["cols_kernel"], a[1]["fft_len"]) == (3, 4, 198750)
    assert _on_the_pair(a[1]) and a[1]["n_bins"] == 26 and a[1]["refine_path"] == 1 and a[1]["n_pairs"] == 1
    assert _on_l_point(b[1]) and b[1]["fft_len"] == 327680
    _same_bits(a, b)
    ref = oacq.acquisition_b2a(x.astype(np.float64), s, coarse=cfast.backend(threads=_cpus()))
    np.testing.assert_array_equal(a[0][1], ref.codePhase)
    np.testing.assert_array_equal(a[0][0], ref.carrFreq)
    np.testing.assert_allclose(a[0][2], ref.peakMetric, rtol=1e-6)
    assert a[0][0][ABSENT - 1] == 0
    for p, bin_ in zip(PRNS, BINS):
        assert a[0][0][p - 1] != 0, p
        assert int(a[6][p - 1]) == bin_ + 1, (p, int(a[6][p - 1]), bin_)  # j = 0 .. 4, m = 0 and 5
        i = prns.index(p)
        assert int(a[3][i][bin_]) == int(a[0][1][p - 1]), p  # the sieve's maximum of the winning cell is the reported code phase
    # the placement itself: the winners sit on the layout's edges ...
    for p, e in zip(PRNS[2:], EDGES):
        t1, t2, t3 = coords(int(a[0][1][p - 1]) - 1)
        assert (t1, t3) == (e[0], e[2]) and t2 in (e[1], (e[1] + 3) % K2), (p, e, (t1, t2, t3))
    assert {coords(int(a[0][1][p - 1]) - 1)[0] for p in PRNS[2:]} >= {0, 52}
    # ... and at the two ends of the 2 ms, where a second-peak range is empty (B2a/acquisition.m:224-249: cp - s2c >= 1, cp + s2c < N)
    for p, cp in ENDS.items():
        assert int(a[0][1][p - 1]) == cp, (p, int(a[0][1][p - 1]))
    assert ENDS[3] - S2C < 1 and ENDS[3] + S2C < N        # PRN 3: no left range
    assert ENDS[11] - S2C >= 1 and not ENDS[11] + S2C < N  # PRN 11: no right range
    assert a[5][3 - 1] > 0 and a[5][11 - 1] > 0           # and a second peak from the range that is left


@pytest.mark.parametrize("step,band,bins", [(250.0, 5000.0, 41), (500.0, 5000.0, 21), (1000.0, 5000.0, 11)])
def test_other_steps_on_the_pair(block, monkeypatch, step, band, bins):
    """acqStep N / fs = 1/2, 1 and 2: two spectra, and whole bins per step"""
    s0, x, sats, _ = block
    s = s0.copy(acqStep=step, acqSearchBand=band)
    prns = [3, 5, 53, 8]
    a = _run(monkeypatch, s, x, prns, True)
    b = _run(monkeypatch, s, x, prns, False)
    assert _on_the_pair(a[1]) and a[1]["n_bins"] == bins and _on_l_point(b[1])
    _same_bits(a, b)
    assert a[0][0][3 - 1] != 0 and a[0][0][53 - 1] != 0 and a[0][0][8 - 1] != 0 and a[0][0][5 - 1] == 0


@pytest.mark.parametrize("change,env,why", [(dict(acqStep=410.0, acqSearchBand=4920.0), None, "410 Hz x 2 ms = 41/50 of a bin"),
                                            (dict(samplingFreq=102e6), None, "another sampling rate: N = 204 000"),
                                            (dict(resamplingflag=1), None, "the search runs on the resampled block"),
                                            (dict(), {"BDS_ACQ_FP16": "0"}, "fp32 storage"),
                                            (dict(), {"BDS_ACQ_HOSTREFINE": "1"}, "refinement through the host"),
                                            (dict(), {"BDS_ACQ_NO_BWREUSE": "1"}, "second-peak pass with a row pass of its own"),
                                            (dict(), {"BDS_ACQ_NEIGH": "1"}, "neighbours refined"),
                                            (dict(), {"BDS_ACQ_PBCAP_GB": "0.05"}, "2 x 26 cells of 1.66 MB do not fit a pair budget of 54 MB")])
def test_settings_the_pair_does_not_cover_take_the_l_point_pair_with_the_switch_on(monkeypatch, change, env, why):
    """Each case stays on the L-point pair with the switch on: rows_kernel in (1, 2), the specialised kernels, and the same kernels, path
    and result bits as with the switch off.  One case asserts rows_kernel in (0, 1, 2) instead: with resamplingflag the search runs on
    the resampled block (48.06 MS/s), whose plan has no specialised kernels, so the run-time-plan kernels of the L-point pair (0) search it
    with the switch on or off -- an L-point run all the same (fft_len and n_circ are not N, and equality with the switch-off run holds)."""
    from helpers import spc_of

    s = bds_amd.init_settings_b2a(acqSatelliteList=[19, 20]).copy(**change)
    spc = spc_of(s)
    x = synth.make_if(s, [synth.Sat(19, 310.0, 0.37 * spc, 1.1, 47.0)], 17 * spc, seed=3550)
    a = _run(monkeypatch, s, x, [19, 20], True, env)
    b = _run(monkeypatch, s, x, [19, 20], False, env)
    if change.get("resamplingflag"):  # (the resampled block, 48.06 MS/s, is searched by the run-time-plan kernels of the L-point pair: 0)
        assert a[1]["rows_kernel"] in (0, 1, 2) and a[1]["fft_len"] != N and a[1]["n_circ"] != N, why
    else:
        assert _on_l_point(a[1]), why
    assert a[0][0][19 - 1] != 0 and a[0][0][20 - 1] == 0
    assert a[1]["fft_len"] == b[1]["fft_len"] and (a[1]["rows_kernel"], a[1]["cols_kernel"], a[1]["refine_path"]) == (b[1]["rows_kernel"], b[1]["cols_kernel"], b[1]["refine_path"])
    for u, v in zip(a[0], b[0]):
        assert np.array_equal(u, v)


MANY = [19, 2, 4, 6, 20, 9, 10, 12, 21, 14, 15, 16, 24, 26, 27, 30]  # 16 PRNs; 19, 20, 21 and 24 present


@pytest.fixture(scope="module")
def one_bin_block():
    """acqSearchBand 0: one Doppler bin at the IF; four satellites within 100 Hz of it"""
    s = bds_amd.init_settings_b2a(acqSatelliteList=sorted(MANY)).copy(acqSearchBand=0.0)
    sats = [synth.Sat(19, 40.0, 0.37 * SPC, 1.1, 50.0), synth.Sat(20, -70.0, 0.81 * SPC, 0.4, 50.0),
            synth.Sat(21, 0.0, delay_of(lag_of(52, 5, 31)), 2.0, 50.0), synth.Sat(24, 95.0, 0.05 * SPC, 0.2, 50.0)]
    x = synth.make_if(s, sats, 17 * SPC, seed=77, code_doppler=False)
    return s, x


def _found(res):
    return set(int(p) for p in np.nonzero(res[0])[0] + 1)


def test_one_doppler_bin_and_nine_or_more_prns(one_bin_block, monkeypatch):
    """acqSearchBand 0 is one bin per PRN: the inter-pass buffer of a fresh context is then its floor of 8 L-point transforms, which holds
    12 cells of this pair (1.66 MB each) but only 8 counted in L-point cells.  The device chain's second-peak pass is admitted by the
    cells of the pair that ran, and the second peaks are the switch-off run's bits."""
    s, x = one_bin_block
    prns = [2, 4, 6, 9, 10, 12, 19, 20, 21, 24]
    a = _run(monkeypatch, s, x, prns, True)
    b = _run(monkeypatch, s, x, prns, False)
    assert _on_the_pair(a[1]) and a[1]["n_bins"] == 1 and a[1]["n_pairs"] == 1 and a[1]["refine_path"] == 1
    assert _on_l_point(b[1])
    _same_bits(a, b)
    assert _found(a[0]) == {19, 20, 21, 24}
    t1, _, t3 = coords(int(a[0][1][21 - 1]) - 1)
    assert (t1, t3) == (52, 31)  # PRN 21 on the last t1 and the last lag of a tile
    assert np.all(a[5][[p - 1 for p in prns]] > 0)  # a second peak for every PRN of the list


@pytest.mark.parametrize("band,nomem,n_pairs,path", [(5000.0, 1, 2, 1), (0.0, 2, 4, 0)])
def test_a_halved_pair_keeps_the_second_peak_pass_on_the_list(block, one_bin_block, monkeypatch, band, nomem, n_pairs, path):
    """The search halves the PRNs per pair when the inter-pass buffer cannot be allocated (BDS_ACQ_TEST_PAIR_NOMEM of the hooks build
    takes the first n allocations to have failed).  The winning cells are then not all in the buffer, and the second-peak pass runs the row
    pass of the listed cells before its masked column pass:
      26 bins, 16 PRNs, 8 per pair: the buffer holds 208 cells, the device chain runs (refine_path 1);
      1 bin, 16 PRNs, 4 per pair: the buffer is its floor of 12 cells < 16, the refinement goes through the host, whose second-peak pass
      walks the list in pieces of 12 and 4 cells (never the L-point kernels: the spectra are in the N-point layout)."""
    if band:
        s0, x, _, _ = block
        s = s0.copy(acqSatelliteList=sorted(set(PRNS + [ABSENT] + MANY))[:16])
        want = set(PRNS) & set(s.acqSatelliteList)
    else:
        s, x = one_bin_block
        want = {19, 20, 21, 24}
    prns = list(s.acqSatelliteList)
    assert len(prns) == 16
    env = {"BDS_ACQ_TEST_PAIR_NOMEM": str(nomem)}
    a = _run(monkeypatch, s, x, prns, True, env)
    b = _run(monkeypatch, s, x, prns, False)
    assert _on_the_pair(a[1]) and a[1]["n_pairs"] == n_pairs and a[1]["refine_path"] == path
    assert _on_l_point(b[1])
    _same_bits(a, b)
    assert _found(a[0]) == want


def test_one_component_b1c_is_not_touched_by_the_switch(monkeypatch):
    """the switch names B2a: a one-component B1C run at the same sampling rate takes the L-point pair with it on"""
    from helpers import spc_of

    s = bds_amd.init_settings_b1c(samplingFreq=99.375e6, IF=14.58e6, acqSatelliteList=[19, 20], acqSearchBand=200.0, pilotACQflag=0)
    spc = spc_of(s)
    x = synth.make_if(s, [synth.Sat(19, -108.0, 0.613 * spc, 0.7, 47.0)], 4 * spc, seed=53)
    a = _run(monkeypatch, s, x, [19, 20], True)
    assert a[1]["rows_kernel"] in (1, 2) and a[1]["n_comp"] == 1 and a[1]["fft_len"] not in (N, 1987500)
    assert a[0][0][19 - 1] != 0 and a[0][0][20 - 1] == 0


def test_all_zero_block_falls_back_and_the_next_block_is_served_again(block):
    """an all-zero block is one exact tie over every lag: the candidate list runs over and the call is redone on the L-point pair with fp32
    storage, then on the run-time-plan kernels: nothing detected, and the next block on the same context starts on the N-point pair again"""
    s, x, sats, _ = block
    c = bds_amd.native.Context(0)
    try:
        c.acq_set_b2a_npoint(True)
        c.acq_load(s, np.zeros(len(x), dtype=np.int8))
        c.acq_prepare(s)
        res = c.acq_run(s, prn_list=[3, 5])
        assert not np.any(res[0]) and not np.any(res[1])
        assert c.timing()["fft_len"] != N
        c.acq_load(s, x)
        c.acq_prepare(s)
        res = c.acq_run(s, prn_list=[3, 5])
        assert _on_the_pair(c.timing())
        assert res[0][3 - 1] != 0 and res[0][5 - 1] == 0
    finally:
        c.close()


def test_b2a_and_b1c_53_msps_alternate_on_one_context(block, monkeypatch):
    """B2a N-point (bds_acq_pfa6.h), B1C at 53 MS/s (bds_acq_pfa32.h), B2a N-point again on one context: the cached code spectra follow the
    layout, each run reports its own pair, the two B2a runs and a fresh context's agree bit for bit; then the switch goes off on the same
    context and the run is the L-point one"""
    from helpers import spc_of

    s2, x2, _, _ = block
    p2 = [3, 5, 53]
    s1 = bds_amd.init_settings_b1c(acqSatelliteList=[19, 20], acqSearchBand=400.0)
    spc1 = spc_of(s1)
    x1 = synth.make_if(s1, [synth.Sat(19, -308.0, 0.613 * spc1, 0.7, 47.0)], 4 * spc1, seed=53)
    c = bds_amd.native.Context(0)
    out = []
    try:
        for s, x, prns in ((s2, x2, p2), (s1, x1, [19, 20]), (s2, x2, p2)):
            out.append(_run(monkeypatch, s, x, prns, True, ctx=c))
        off = _run(monkeypatch, s2, x2, p2, False, ctx=c)
        on_again = _run(monkeypatch, s2, x2, p2, True, ctx=c)
    finally:
        c.close()
    assert [o[1]["fft_len"] for o in out] == [N, 1060000, N]
    assert [(o[1]["rows_kernel"], o[1]["cols_kernel"]) for o in out] == [(3, 4)] * 3
    assert (out[0][1]["plan_l1"], out[0][1]["plan_l2"], out[1][1]["plan_l1"], out[1][1]["plan_l2"]) == (318, 625, 53 * 32, 625)
    assert _on_l_point(off[1]) and _on_the_pair(on_again[1])
    fresh = _run(monkeypatch, s2, x2, p2, True)
    for other in (out[2], on_again, fresh):
        _same_bits(out[0], other)
        np.testing.assert_array_equal(out[0][2], other[2])
        np.testing.assert_array_equal(out[0][3], other[3])
    _same_bits(out[0], off)
    assert out[1][0][0][19 - 1] != 0 and out[1][0][0][20 - 1] == 0


def test_iq_record(monkeypatch):
    """fileType 2 (interleaved I/Q int8, B2a/postProcessing.m:92-96): the complex block through the N-point pair"""
    from helpers import cfg1_b2a_iq

    s, x, sats = cfg1_b2a_iq()
    a = _run(monkeypatch, s, x, [19, 20, 21], True, is_complex=True)
    b = _run(monkeypatch, s, x, [19, 20, 21], False, is_complex=True)
    assert _on_the_pair(a[1]) and a[1]["n_bins"] == 5 and _on_l_point(b[1])
    _same_bits(a, b)
    assert a[0][0][19 - 1] != 0 and a[0][0][20 - 1] != 0 and a[0][0][21 - 1] == 0


def test_acquisition_keyword_and_a_part_of_the_prn_list(block):
    """bds_amd.acquisition(..., b2a_npoint=True) sets the process-wide context's switch; a shard of the PRN list runs on the pair too"""
    s, x, sats, _ = block
    try:
        on = bds_amd.acquisition(x, s, prn_list=[3, 5], verbose=False, b2a_npoint=True)
        assert _on_the_pair(bds_amd.get_context(0).timing())
        off = bds_amd.acquisition(x, s, prn_list=[3, 5], verbose=False, b2a_npoint=False)
        assert _on_l_point(bds_amd.get_context(0).timing())
    finally:
        bds_amd.get_context(0).acq_set_b2a_npoint(False)
    for f in ("carrFreq", "codePhase", "peakMetric"):
        np.testing.assert_array_equal(getattr(on, f), getattr(off, f))
    assert on.carrFreq[3 - 1] != 0 and on.carrFreq[5 - 1] == 0


def test_cfg2_full_size_switch_on_against_switch_off(monkeypatch):
    """BASELINE.json configs[1], all 63 PRNs x 26 bins in one launch pair (2.7 GB)"""
    import bench

    s, x, sats, _ = bench.build_workload("b2a")
    prns = list(s.acqSatelliteList)
    a = _run(monkeypatch, s, x, prns, True)
    b = _run(monkeypatch, s, x, prns, False)
    assert _on_the_pair(a[1]) and a[1]["n_prn"] == 63 and a[1]["n_pairs"] == 1 and a[1]["refine_path"] == 1
    assert _on_l_point(b[1])
    _same_bits(a, b)
    assert set(np.nonzero(a[0][0])[0] + 1) == {sat.prn for sat in sats}
