"""The position fix on the GPU against the restatement of tests/pvt_cases.py: bds_pvt_measure at four shapes (transmitTime bit-equal,
satPos within 1e-6 m, satClkCorr within 1e-16 s), the whole chain through bds_post_navigation on the host test's cases, and
post_navigation from prompt series -- decoding, readiness, measurement, fix -- against the restatement and the true position.

Tolerances (the table of pvt_cases.compare_solutions for the chain):
    transmitTime  bit-equal   only IEEE + - * /
    satPos        1e-6 m      ~1 ulp errors of sin, cos and atan2 reach E and u as ~3e-15 rad, times 4.2e7 m ~ 1.3e-7 m; 8x margin
    satClkCorr    1e-16 s     its ulp is ~1e-20 s
"""
import numpy as np
import pytest

import bds_amd
import pvt_cases as pc
from bds_amd import native

pytestmark = pytest.mark.gpu

C_LIGHT = 299792458.0

# (signal, n_ch, n, n_meas, navSolPeriod [ms]): the period only has to let the plan give n_meas epochs
SHAPES = [("B1C", 4, 40, 1, 200), ("B1C", 5, 64, 7, 50), ("B2A", 33, 257, 65, 2), ("B1C", 12, 3700, 180, 200)]
_MEASURE = {}


def measure_case(signal, n_ch, n, n_meas, period):
    """The scenario of a shape with the places a kernel can go wrong written into it; built once."""
    key = (signal, n_ch, n, n_meas)
    if key in _MEASURE:
        return _MEASURE[key]
    scn = pc.make_scenario(signal, n_ch, n, overrides=dict(navSolPeriod=period), seed=40 + n_ch)
    p = pc.plan(scn.settings, scn.status, scn.absoluteSample, scn.ephs, scn.subFrameStart, scn.TOW)
    assert p["n_meas"] >= n_meas and (p["ready"] == pc.READY).all()
    ready = p["ready"].copy()
    ready[1] = pc.NO_EPH  # a channel that is not ready: NaN
    ephs, tow = [dict(e) for e in scn.ephs], scn.TOW.copy()
    tow[2] = 500004.0  # time - t_oe > 302400: the first branch of check_t
    ephs[3]["t_oe"] = ephs[3]["t_oc"] = 604500.0  # time - t_oe < -302400: the second
    # epoch 0 falls ON an entry of channel 0's absoluteSample (that entry belongs to the next interval) ...
    c0, k0 = 0, int(max(scn.subFrameStart)) + 2
    start = scn.absoluteSample[c0, k0]
    assert start >= p["sampleStart"]
    # ... and the last epoch lies past every channel's last entry: index = n - 1
    step = p["measSampleStep"] if n_meas == 1 else float(np.ceil((scn.absoluteSample[:, -1].max() + 5 - start) / (n_meas - 1)))
    want = pc.measure(scn.settings, ready, scn.absoluteSample, scn.codeFreq, scn.remCodePhase, ephs, scn.subFrameStart, tow, start, step, n_meas)
    idx = want[3]
    assert idx[0, c0] == k0 + 1 and pc.index_scan(scn.absoluteSample[c0], start) == k0 + 1
    if n_meas > 1:
        assert (idx[-1, ready == pc.READY] == n - 1).all() and (idx[-2, ready == pc.READY] < n - 1).any()
    # both branches of check_t, a negative Phi, e = 0 and e = 0.02, MEO and IGSO
    tr = [{} for _ in range(n_ch)]
    for c in range(n_ch):
        pc.satpos(want[0][:, c] if ready[c] & pc.READY else np.array([tow[c]]), ephs[c], signal == "B1C", trace=tr[c])
    assert (tr[2]["raw_tk"] > pc.HALF_WEEK).all() and (tr[3]["raw_tk"] < -pc.HALF_WEEK).all()
    assert any((t["Phi"] < 0).any() for t in tr) and any((t["Phi"] > 0).any() for t in tr)
    assert {e["e"] == 0 for e in ephs} == {True, False}
    if n_ch >= 5:
        assert {e["SatType"] for e in ephs} == {pc.MEO, pc.IGSO}
    if signal == "B2A":
        assert all(np.isnan(e["T_GDB1Cp"]) for e in ephs)
    _MEASURE[key] = (scn, ready, ephs, tow, start, step, want)
    return _MEASURE[key]


@pytest.mark.parametrize("signal,n_ch,n,n_meas,period", SHAPES)
def test_measure_against_the_restatement(ctx, signal, n_ch, n, n_meas, period):
    scn, ready, ephs, tow, start, step, want = measure_case(signal, n_ch, n, n_meas, period)
    tt, sp, ck = ctx.pvt_measure(scn.settings, ready, scn.absoluteSample, scn.codeFreq, scn.remCodePhase, ephs, scn.subFrameStart, tow,
                                 start, step, n_meas)
    on = ready == pc.READY
    assert np.isnan(tt[:, ~on]).all() and np.isnan(sp[:, ~on]).all() and np.isnan(ck[:, ~on]).all()
    assert np.isfinite(want[0][:, on]).all() and np.isfinite(want[1][:, on]).all()
    d_pos, d_clk = np.abs(sp[:, on] - want[1][:, on]).max(), np.abs(ck[:, on] - want[2][:, on]).max()
    n_tt = int((tt[:, on] != want[0][:, on]).sum())
    print(f"measure {signal} {n_ch} x {n} x {n_meas}: transmitTime differs at {n_tt}, satPos worst {d_pos:.3e} m, satClkCorr worst {d_clk:.3e} s")
    np.testing.assert_array_equal(tt, want[0])  # bit-equal, NaN in the same places
    assert d_pos <= 1e-6 and d_clk <= 1e-16


def test_measure_refuses_bad_arguments(ctx):
    scn, ready, ephs, tow, start, step, _ = measure_case(*SHAPES[0])
    with pytest.raises(native.BdsError, match="empty SatType"):
        ctx.pvt_measure(scn.settings, [1, 1, 1, 1], scn.absoluteSample, scn.codeFreq, scn.remCodePhase, [dict(ephs[0], SatType=0)] + ephs[1:],
                        scn.subFrameStart, tow, start, step, 1)
    with pytest.raises(native.BdsError, match="must be positive"):
        ctx.pvt_measure(scn.settings.copy(codeFreqBasis=0.0), ready, scn.absoluteSample, scn.codeFreq, scn.remCodePhase, ephs,
                        scn.subFrameStart, tow, start, step, 1)
    tt, sp, ck = ctx.pvt_measure(scn.settings, ready, scn.absoluteSample, scn.codeFreq, scn.remCodePhase, ephs, scn.subFrameStart, tow,
                                 start, step, 0)
    assert tt.shape == (0, 4) and sp.shape == (0, 4, 3)


@pytest.mark.parametrize("name", ["b1c_5x7", "b1c_5x7_notrop", "b1c_4x1", "low_of_5", "low_of_4", "duplicate_prn", "b2a_6", "idle_and_no_eph"])
def test_post_navigation_entry_on_the_host_cases(ctx, name):
    scn = pc.host_cases()[name]
    p, _, want = pc.run_reference(scn)
    got, ready = ctx.post_navigation(scn.settings, scn.status, scn.prns, scn.absoluteSample, scn.codeFreq, scn.remCodePhase, scn.ephs,
                                     scn.subFrameStart, scn.TOW)
    np.testing.assert_array_equal(ready, p["ready"])
    assert got["X"].shape == (p["n_meas"],)
    print(name, pc.compare_solutions(got, want))


def test_post_navigation_entry_without_a_solution(ctx):
    scn = pc.host_cases()["b1c_5x7"]
    got, ready = ctx.post_navigation(scn.settings, "T-T-T", scn.prns, scn.absoluteSample, scn.codeFreq, scn.remCodePhase, scn.ephs,
                                     scn.subFrameStart, scn.TOW)
    assert got is None and list(ready) == [1, 2, 1, 2, 1]
    got, ready = ctx.post_navigation(scn.settings.copy(navSolPeriod=1000), scn.status, scn.prns, scn.absoluteSample, scn.codeFreq,
                                     scn.remCodePhase, scn.ephs, scn.subFrameStart, scn.TOW)
    assert got is None and (ready == 1).all()
    bad = scn.absoluteSample.copy()
    bad[0, 5] = bad[0, 4]
    with pytest.raises(native.BdsError, match="strictly increasing"):
        ctx.post_navigation(scn.settings, scn.status, scn.prns, bad, scn.codeFreq, scn.remCodePhase, scn.ephs, scn.subFrameStart, scn.TOW)


def _from_prompts(signal, n, seed, **overrides):
    scn = pc.make_scenario(signal, 5, n, overrides=dict(useTropCorr=0, **overrides), seed=seed)
    assert len(set(scn.subFrameStart)) > 1  # the frames start at different indices
    rows = pc.track_results(scn, np.random.default_rng(seed))
    nav, eph = bds_amd.post_navigation(rows, scn.settings)
    p, _, want = pc.run_reference(scn)
    assert nav is not None and (nav.channelStatus == pc.READY).all() and nav.X.shape == (p["n_meas"],)
    # the decoded ephemerides are the scenario's, by PRN
    assert sorted(eph) == sorted(int(x) for x in scn.prns)
    for c, prn in enumerate(scn.prns):
        for f in ("M_0", "e", "omega_0", "t_oe", "a_0", "deltaA"):
            assert getattr(eph[int(prn)], f) == scn.ephs[c][f]
    print(signal, "from prompts", pc.compare_solutions(vars(nav), want))
    err = np.sqrt((nav.X - scn.rx[0]) ** 2 + (nav.Y - scn.rx[1]) ** 2 + (nav.Z - scn.rx[2]) ** 2)
    bound = np.array([pc.truth_bound(A, scn.tow, C_LIGHT) for A in want["A"]])
    print(signal, "from prompts: worst error against the true position / bound [m]", err.max(), bound.min())
    assert (err <= bound).all()
    return scn, rows


def test_post_navigation_from_prompts_b1c(ctx):
    scn, rows = _from_prompts("B1C", 3700, 61, msToProcess=37000, pilotTRKflag=2)
    assert bds_amd.postNavigation is bds_amd.post_navigation
    # the record-length gate (postNavigation.m:49)
    assert bds_amd.post_navigation(rows, scn.settings.copy(msToProcess=35999)) == (None, None)
    # an idle row in between keeps its channel number; three ready channels are no solution, the ephemerides still come back
    idle = pc.SimpleNamespace(PRN=0, status="-")
    nav, eph = bds_amd.post_navigation(rows[:2] + [idle] + rows[2:], scn.settings.copy(numberOfChannels=6))
    assert nav.PRN.shape[0] == 6 and (nav.PRN[2] == 0).all() and list(nav.channelStatus) == [1, 1, 2, 1, 1, 1]
    nav, eph = bds_amd.post_navigation(rows[:3], scn.settings)
    assert nav is None and len(eph) == 3
    with pytest.raises(AttributeError, match="elevationMask"):
        s = scn.settings.copy()
        del s.elevationMask
        bds_amd.post_navigation(rows, s)


def test_post_navigation_from_prompts_b2a(ctx):
    scn, rows = _from_prompts("B2A", 12200, 62)
    assert all(list(e["idValid"][:3]) == [10, 11, 30] for e in scn.ephs)
    assert bds_amd.post_navigation(rows, scn.settings.copy(msToProcess=23999)) == (None, None)
