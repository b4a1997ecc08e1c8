"""The N-point search pair at 53 MS/s (csrc/bds_acq_pfa32.h: B1C at N = 1 060 000 = 53 x 32 x 625, the settings of the reference's own
B1C/initSettings.m and the defaults of init_settings_b1c()): which settings take it, and that every one of them decides what the L-point
pair (BDS_ACQ_PFA=0) decides.  The whole 201-bin grid against the float64 oracle at this rate lives in tests/test_fullsize_gpu.py
(test_b1c_at_the_references_own_sampling_rates_against_the_c_oracle[53MSps, 53MSps-IQ] runs on this pair by default)."""
import numpy as np
import pytest

import bds_amd
from bds_amd import synth

pytestmark = pytest.mark.gpu
N = 1060000
N3 = 1987500
K1, K2, K3 = 53, 32, 625
TILE = 8  # lags t3 per tile of the inter-pass buffer (pfa32::kTileLags)


def _run(monkeypatch, s, x, prns, env=None, is_complex=None):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    c = bds_amd.native.Context(0)  # the knobs are read once, at context creation
    for k in (env or {}):
        monkeypatch.delenv(k)
    try:
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
        c.close()
    return res, tm, grid, arg, pk, fb


def _same_decisions(a, b):
    for u, v in zip(a[0], b[0]):
        assert np.array_equal(u, v)          # carrFreq, codePhase, peakMetric (f64 decisions): bit for bit
    np.testing.assert_array_equal(a[4], b[4])  # f64 peaks
    np.testing.assert_array_equal(a[5], b[5])  # winning bins
    np.testing.assert_allclose(a[2], b[2], rtol=2e-3)  # the two sieves' row maxima: within kDelta / 2 of each other


def _on_the_new_pair(tm):
    return (tm["rows_kernel"], tm["cols_kernel"], tm["fft_len"], tm["plan_l1"], tm["plan_l2"]) == (3, 4, N, K1 * K2, K3)


@pytest.fixture(scope="module")
def block():
    """40 ms at the default settings: PRN 19 at -308 Hz, PRN 35 at +210 Hz, PRN 46 at +13.77 kHz; PRN 20 absent"""
    from helpers import spc_of

    s = bds_amd.init_settings_b1c()
    assert (s.samplingFreq, s.IF, s.acqCohT, s.acqStep, s.pilotACQflag) == (53e6, 1590e6 - 1575.42e6, 10, 50, 1)
    spc = spc_of(s)
    sats = [synth.Sat(19, -308.0, 0.613 * spc, 0.7, 47.0), synth.Sat(35, 210.0, 0.2 * spc, 2.0, 46.0), synth.Sat(46, 13770.0, 0.41 * spc, 1.1, 47.0)]
    return s.copy(acqSatelliteList=list(range(1, 64))), synth.make_if(s, sats, 4 * spc, seed=53)


def test_the_default_settings_take_the_n_point_pair(block, monkeypatch):
    """init_settings_b1c() as it stands, a +-400 Hz band (17 bins), three PRNs: the call reports the pair of bds_acq_pfa32.h on N points,
    the L-point pair another transform length, and both decide the same"""
    s0, x = block
    s = s0.copy(acqSearchBand=400.0)
    prns = [19, 20, 35]
    a = _run(monkeypatch, s, x, prns)
    b = _run(monkeypatch, s, x, prns, {"BDS_ACQ_PFA": "0"})
    assert (a[1]["rows_kernel"], a[1]["cols_kernel"], a[1]["fft_len"]) == (3, 4, 1060000)
    assert _on_the_new_pair(a[1]) and a[1]["n_bins"] == 17
    assert b[1]["fft_len"] != N and b[1]["fft_len"] > N and b[1]["rows_kernel"] in (1, 2)
    _same_decisions(a, b)
    assert a[0][0][19 - 1] != 0 and a[0][0][35 - 1] != 0 and a[0][0][20 - 1] == 0
    assert abs(a[0][0][19 - 1] - (s.IF - 308.0)) <= 25


def test_doppler_steps_of_two_bins_and_a_shifted_band(block, monkeypatch):
    """acqStep = 100 Hz is two spectrum bins per Doppler bin (acqStep N / fs = 2); a +-950 Hz band moves the first bin's frequency"""
    s0, x = block
    s = s0.copy(acqStep=100.0, acqSearchBand=950.0)
    prns = [19, 20, 35]
    a = _run(monkeypatch, s, x, prns)
    b = _run(monkeypatch, s, x, prns, {"BDS_ACQ_PFA": "0"})
    assert _on_the_new_pair(a[1]) and a[1]["n_bins"] == 20 and b[1]["fft_len"] != N
    _same_decisions(a, b)
    assert a[0][0][19 - 1] != 0 and a[0][0][35 - 1] != 0 and a[0][0][20 - 1] == 0


def test_rotation_past_625(block, monkeypatch):
    """a +-31.3 kHz band in steps of 100 Hz: 627 bins, the last one a rotation by 1252 spectrum bins -- past 625 twice, so that s mod 53,
    s mod 32 and s mod 625 all differ from s; PRN 46 sits at +13.77 kHz (rotation 902)"""
    s0, x = block
    s = s0.copy(acqStep=100.0, acqSearchBand=31300.0)
    prns = [46]
    a = _run(monkeypatch, s, x, prns)
    b = _run(monkeypatch, s, x, prns, {"BDS_ACQ_PFA": "0"})
    assert _on_the_new_pair(a[1]) and a[1]["n_bins"] == 627 and b[1]["fft_len"] != N
    assert 2 * (a[1]["n_bins"] - 1) >= 2 * K3
    _same_decisions(a, b)
    assert a[0][0][46 - 1] != 0 and abs(a[0][0][46 - 1] - (s.IF + 13770.0)) <= 50
    assert int(a[5][46 - 1]) * 2 > K3  # (the winning bin's rotation is itself past 625)


EDGES = [(0, 0, 0), (52, 31, 624), (26, 15, 7), (1, 16, 8), (51, 17, 623), (13, 1, 616)]


def test_peaks_on_the_edges_of_the_three_dimensions(monkeypatch):
    """six satellites whose correlation peaks sit at the first / last index of the 53-, 32- and 625-point dimensions, on both sides of the
    column pass's split of the 32 (t2 = 15 / 16 / 17) and of the inter-pass buffer's tile boundaries (lag in the tile 7 / 0, the last
    tile's single lag 624): lag = t1 N/53 + t2 N/32 + t3 N/625 mod N"""
    from helpers import spc_of

    s = bds_amd.init_settings_b1c(acqSatelliteList=list(range(1, 64)), acqSearchBand=1000.0)
    spc = spc_of(s)
    lags = [(t1 * (N // K1) + t2 * (N // K2) + t3 * (N // K3)) % N for t1, t2, t3 in EDGES]
    assert [(t % K3) // TILE for t in (7, 8, 616, 623, 624)] == [0, 1, 77, 77, 78]
    prns = [3, 11, 17, 29, 41, 53]
    # (the sieve's maximum of a synthetic satellite sits two samples behind the sample its code period starts at: the reference's sampled
    #  code tables index with ceil(), B1C/acquisition.m:150-160)
    sats = [synth.Sat(p, 50.0 * (5 * i - 12), float((t - LOBE) % spc), 0.3 + i, 50.0) for i, (p, t) in enumerate(zip(prns, lags))]
    x = synth.make_if(s, sats, 4 * spc, seed=41, code_doppler=False)
    a = _run(monkeypatch, s, x, prns + [5])
    b = _run(monkeypatch, s, x, prns + [5], {"BDS_ACQ_PFA": "0"})
    assert _on_the_new_pair(a[1]) and b[1]["fft_len"] != N
    _same_decisions(a, b)
    for i, (p, t) in enumerate(zip(prns, lags)):
        assert a[0][0][p - 1] != 0, p
        bin_ = int(np.argmax(a[2][i]))
        assert int(a[3][i][bin_]) % spc == t % spc == int(b[3][i][bin_]) % spc, (p, EDGES[i], int(a[3][i][bin_]), t)
        d = (a[0][1][p - 1] - t) % spc
        assert min(d, spc - d) <= 3.0, (p, a[0][1][p - 1], t % spc)
    assert a[0][0][4] == 0


LOBE = 2  # samples between a synthetic satellite's code-period start and the sieve's maximum at 53 MS/s


def test_iq_record(monkeypatch):
    """fileType 2 (interleaved I/Q int8, B1C/postProcessing.m:92-96) at 53 MS/s: the complex block through the N-point pair"""
    from bds_amd.acquisition import _as_int8
    from helpers import as_complex, spc_of

    s = bds_amd.init_settings_b1c(acqSatelliteList=list(range(1, 64)), fileType=2, acqSearchBand=2000.0)
    spc = spc_of(s)
    sats = [synth.Sat(7, -1730.0, 0.613 * spc, 0.7, 45.0), synth.Sat(23, 1210.0, 0.2 * spc, 2.0, 46.0)]
    x, is_complex = _as_int8(as_complex(synth.make_if(s, sats, 4 * spc, seed=77, iq_sign=-1)), s)
    assert is_complex
    prns = [7, 8, 23]
    a = _run(monkeypatch, s, x, prns, is_complex=True)
    b = _run(monkeypatch, s, x, prns, {"BDS_ACQ_PFA": "0"}, is_complex=True)
    assert _on_the_new_pair(a[1]) and a[1]["n_bins"] == 81 and b[1]["fft_len"] != N
    _same_decisions(a, b)
    assert a[0][0][6] != 0 and a[0][0][22] != 0 and a[0][0][7] == 0
    assert abs(a[0][0][6] - (s.IF - 1730.0)) <= 25


@pytest.mark.parametrize("change,why", [(dict(acqCohT=5), "N = 15 ms of samples"),
                                        (dict(pilotACQflag=0), "one component"),
                                        (dict(acqStep=25.0, acqSearchBand=500.0), "half a spectrum bin per Doppler step"),
                                        (dict(resamplingflag=1), "the search runs on the resampled block"),
                                        (dict(samplingFreq=30.69e6), "N = 613 800 = 2^3 3^2 5^2 11 31")])
def test_settings_the_n_point_pair_does_not_cover_take_the_l_point_pair(monkeypatch, change, why):
    from helpers import spc_of

    s = bds_amd.init_settings_b1c(acqSearchBand=500.0).copy(**change)
    spc = spc_of(s)
    x = synth.make_if(s, [synth.Sat(19, -308.0, 0.613 * spc, 0.7, 47.0)], 4 * spc, seed=53)
    res, tm, *_ = _run(monkeypatch, s, x, [19, 20])
    assert res[0][19 - 1] != 0 and res[0][20 - 1] == 0
    assert tm["rows_kernel"] in (1, 2) and tm["fft_len"] not in (N, N3), why


def test_all_zero_block_falls_back_and_the_next_block_is_served_again(block):
    """an all-zero block is one exact tie over every lag: the candidate list runs over and the call is redone on the L-point pair with fp32
    storage, then on the run-time-plan kernels: nothing detected, and the next block on the same context starts on the N-point pair again"""
    s0, x = block
    s = s0.copy(acqSearchBand=400.0)
    c = bds_amd.native.Context(0)
    try:
        c.acq_load(s, np.zeros(len(x), dtype=np.int8))
        c.acq_prepare(s)
        res = c.acq_run(s, prn_list=[1, 2])
        assert not np.any(res[0]) and not np.any(res[1])
        assert c.timing()["fft_len"] != N
        c.acq_load(s, x)
        c.acq_prepare(s)
        res = c.acq_run(s, prn_list=[19, 2])
        assert _on_the_new_pair(c.timing())
        assert res[0][19 - 1] != 0 and res[0][1] == 0
    finally:
        c.close()


def test_cfg3_and_53_msps_in_one_context(block, monkeypatch):
    """99.375 MS/s (bds_acq_pfa.h), 53 MS/s (bds_acq_pfa32.h), 99.375 MS/s again on one context: the cached code spectra are dropped when the
    layout changes, each run reports its own pair, and the two cfg3 runs and a fresh context's agree bit for bit"""
    import bench

    s53, x53 = block
    s53 = s53.copy(acqSearchBand=400.0)
    s3, x3, sats3, _ = bench.build_workload("b1c")
    s3 = s3.copy(acqSearchBand=400.0)
    p3 = [46, 5]  # PRN 46 is in the bench block at -308 Hz, PRN 5 is not
    c = bds_amd.native.Context(0)
    out = []
    try:
        for s, x, prns in ((s3, x3, p3), (s53, x53, [19, 20]), (s3, x3, p3)):
            c.acq_load(s, x)
            c.acq_prepare(s)
            res = c.acq_run(s, prn_list=prns)
            tm = c.timing()
            grid, arg = c.acq_grid(len(prns), int(tm["n_bins"]))
            out.append((res, tm, grid.copy(), arg.copy()))
    finally:
        c.close()
    assert [o[1]["fft_len"] for o in out] == [N3, N, N3]
    assert [(o[1]["rows_kernel"], o[1]["cols_kernel"]) for o in out] == [(3, 4)] * 3
    assert (out[0][1]["plan_l1"], out[0][1]["plan_l2"], out[1][1]["plan_l1"], out[1][1]["plan_l2"]) == (53 * 12, 3125, 53 * 32, 625)
    for u, v in zip(out[0][0], out[2][0]):
        assert np.array_equal(u, v)
    np.testing.assert_array_equal(out[0][2], out[2][2])
    np.testing.assert_array_equal(out[0][3], out[2][3])
    fresh = _run(monkeypatch, s3, x3, p3)
    for u, v in zip(out[0][0], fresh[0]):
        assert np.array_equal(u, v)
    np.testing.assert_array_equal(out[0][2], fresh[2])
    assert out[0][0][0][46 - 1] != 0 and out[0][0][0][4] == 0
    assert out[1][0][0][19 - 1] != 0 and out[1][0][0][20 - 1] == 0
    fresh53 = _run(monkeypatch, s53, x53, [19, 20])
    for u, v in zip(out[1][0], fresh53[0]):
        assert np.array_equal(u, v)
    np.testing.assert_array_equal(out[1][2], fresh53[2])
