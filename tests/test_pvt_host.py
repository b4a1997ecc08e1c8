"""bds_pvt_plan and bds_pvt_solve (host C++, no GPU, through ctypes) against the restatement of tests/pvt_cases.py, on the
restatement's own measurement arrays.  The active lists (PRN), the NaN / +-inf / 0 places and currMeasSample must be identical;
the tolerances of everything else are the table in pvt_cases.compare_solutions."""
import math

import numpy as np
import pytest

import pvt_cases as pc
from bds_amd import native

MASK = 5.0


def _plan(scn, settings=None):
    return native.pvt_plan(settings or scn.settings, scn.status, scn.absoluteSample, scn.ephs, scn.subFrameStart, scn.TOW)


def _same_plan(got, want):
    np.testing.assert_array_equal(got["ready"], want["ready"])
    assert got["n_meas"] == want["n_meas"] and got["measSampleStep"] == want["measSampleStep"]
    for k in ("sampleStart", "sampleEnd"):
        assert got[k] == want[k] or (math.isnan(got[k]) and math.isnan(want[k])), k


def _chain(scn, n_meas=None):
    """(restatement's solution, library's solution on the restatement's measurement arrays)."""
    p, meas, want = pc.run_reference(scn, n_meas=n_meas)
    _same_plan(_plan(scn), p)
    tt, sp, ck, _ = meas
    got = native.pvt_solve(scn.settings, scn.prns, p["ready"], p["sampleStart"], p["measSampleStep"], tt, sp, ck)
    return want, got


def _inputs_are_fair(want):
    """No elevation within 0.01 degrees of the mask, cond(A) <= 50: the conditions under which the tolerances hold."""
    el = want["el"][np.isfinite(want["el"]) & (want["el"] != 0)]
    assert (np.abs(el - MASK) > 0.01).all()
    for A in want["A"]:
        if A is not None and pc.matlab_rank(A) == 4:
            assert np.linalg.cond(A) <= 50


@pytest.mark.parametrize("name,n_meas,epochs_with_fix", [("b1c_5x7", 7, 7), ("b1c_5x7_notrop", 7, 7), ("b1c_4x1", 1, 1), ("b2a_6", 5, 5)])
def test_solve_follows_the_restatement(name, n_meas, epochs_with_fix):
    scn = pc.host_cases()[name]
    want, got = _chain(scn, n_meas)
    assert want["X"].shape == (n_meas,) and np.isfinite(want["X"]).sum() == epochs_with_fix
    _inputs_are_fair(want)
    print(name, pc.compare_solutions(got, want))
    if name == "b1c_5x7":  # the troposphere is in: the two settings differ by metres
        other = pc.run_reference(pc.host_cases()["b1c_5x7_notrop"], n_meas=n_meas)[2]
        assert np.abs(other["X"] - want["X"]).max() > 1.0


def test_low_satellite_is_used_once_and_masked_for_good():
    scn = pc.host_cases()["low_of_5"]
    want, got = _chain(scn, 6)
    assert 2.0 < want["el"][2, 0] < 4.0 and want["active"][0] == [0, 1, 2, 3, 4]
    assert all(a == [0, 1, 3, 4] for a in want["active"][1:]) and np.isfinite(want["X"]).all()
    assert np.isnan(want["el"][2, 1:]).all() and (want["rawP"][2, 1:] == -np.inf).all() and (want["correctedP"][2, 1:] == 0).all()
    _inputs_are_fair(want)
    print("low_of_5", pc.compare_solutions(got, want))


def test_masking_that_leaves_three_gives_nan_rows_and_zero_dop():
    scn = pc.host_cases()["low_of_4"]
    want, got = _chain(scn, 5)
    assert np.isfinite(want["X"][0]) and np.isnan(want["X"][1:]).all() and (want["DOP"][:, 1:] == 0).all()
    assert all(a == [0, 2, 3] for a in want["active"][1:])
    # PRN, transmitTime, satClkCorr and rawP of the three are still stored; el / az are NaN; satElev is not updated
    assert (want["PRN"][[0, 2, 3], 1:] != 0).all() and np.isfinite(want["rawP"][[0, 2, 3], 1:]).all() and np.isnan(want["el"][:, 1:]).all()
    _inputs_are_fair(want)
    print("low_of_4", pc.compare_solutions(got, want))
    assert np.isnan(got["localTime"][1:]).all() and np.isnan(got["currMeasSample"][1:]).all()


def test_duplicate_prn_among_four_takes_the_rank_exit():
    scn = pc.host_cases()["duplicate_prn"]
    assert scn.prns[0] == scn.prns[3]
    want, got = _chain(scn, 3)
    # leastSquarePos.m:90-95 in the first iteration: pos = 0, dop = inf, el = az = 0; cart2geo(0, 0, 0) = NaN, 0, NaN;
    # with el = 0 the mask empties the list from the second epoch on
    assert (want["X"][0], want["Y"][0], want["Z"][0], want["dt"][0], want["longitude"][0]) == (0, 0, 0, 0, 0)
    assert np.isinf(want["DOP"][:, 0]).all() and (want["el"][:, 0] == 0).all() and (want["az"][:, 0] == 0).all()
    assert np.isnan(want["latitude"][0]) and np.isnan(want["height"][0]) and np.isfinite(want["correctedP"][:, 0]).all()
    assert want["active"][1:] == [[], []] and np.isnan(want["X"][1:]).all() and (want["rawP"][:, 1:] == -np.inf).all()
    assert (want["PRN"][:, 0] == scn.prns).all() and (want["PRN"][:, 1:] == 0).all()
    print("duplicate_prn", pc.compare_solutions(got, want))


def test_idle_and_not_ready_channels():
    scn = pc.host_cases()["idle_and_no_eph"]
    p = _plan(scn)
    assert list(p["ready"]) == [pc.READY, pc.READY, pc.IDLE, pc.READY, pc.NO_EPH, pc.READY]
    want, got = _chain(scn, 4)
    assert all(a == [0, 1, 3, 5] for a in want["active"]) and (want["PRN"][[2, 4]] == 0).all() and np.isnan(want["el"][[2, 4]]).all()
    _inputs_are_fair(want)
    print("idle_and_no_eph", pc.compare_solutions(got, want))


def test_b2a_readiness_rule():
    scn = pc.host_cases()["b2a_6"]
    assert all(list(e["idValid"][:3]) == [10, 11, 30] for e in scn.ephs) and all(math.isnan(e["T_GDB1Cp"]) for e in scn.ephs)
    base = _plan(scn)
    assert (base["ready"] == pc.READY).all() and base["n_meas"] >= 5
    for slot, value, ok in [(0, 0, False), (1, 0, False), (2, 0, False), (2, 31, False)]:
        e = dict(scn.ephs[1], idValid=np.array(scn.ephs[1]["idValid"]))
        e["idValid"][slot] = value
        ephs = scn.ephs[:1] + [e] + scn.ephs[2:]
        got = native.pvt_plan(scn.settings, scn.status, scn.absoluteSample, ephs, scn.subFrameStart, scn.TOW)
        _same_plan(got, pc.plan(scn.settings, scn.status, scn.absoluteSample, ephs, scn.subFrameStart, scn.TOW))
        assert (got["ready"][1] == pc.READY) == ok and got["ready"][1] == pc.NO_EPH
    # any one of the clock messages 30 .. 34, in its own slot, will do
    e = dict(scn.ephs[1], idValid=np.array([10, 11, 0, 0, 0, 0, 34, 0]))
    assert native.pvt_plan(scn.settings, scn.status, scn.absoluteSample, scn.ephs[:1] + [e] + scn.ephs[2:], scn.subFrameStart,
                           scn.TOW)["ready"][1] == pc.READY
    # B1C's rule does not apply to B2a: flag is not looked at
    e = dict(scn.ephs[1], flag=0)
    assert native.pvt_plan(scn.settings, scn.status, scn.absoluteSample, scn.ephs[:1] + [e] + scn.ephs[2:], scn.subFrameStart,
                           scn.TOW)["ready"][1] == pc.READY


def test_plan_without_a_solution():
    scn = pc.host_cases()["b1c_5x7"]
    # fewer than 4 ready: two idle of five
    st = "T-T-T"
    got = native.pvt_plan(scn.settings, st, scn.absoluteSample, scn.ephs, scn.subFrameStart, scn.TOW)
    _same_plan(got, pc.plan(scn.settings, st, scn.absoluteSample, scn.ephs, scn.subFrameStart, scn.TOW))
    assert got["n_meas"] == 0 and math.isnan(got["sampleStart"]) and list(got["ready"]) == [1, 2, 1, 2, 1]
    # n_meas <= 0: the record ends before one step fits
    s = scn.settings.copy(navSolPeriod=1000)
    got = _plan(scn, s)
    _same_plan(got, pc.plan(s, scn.status, scn.absoluteSample, scn.ephs, scn.subFrameStart, scn.TOW))
    assert got["n_meas"] == 0 and got["sampleEnd"] > got["sampleStart"] and (got["ready"] == 1).all()
    # ... or before the latest sub-frame start (a negative quotient)
    sfs = scn.subFrameStart.copy()
    sfs[0] = scn.n
    got = native.pvt_plan(scn.settings, scn.status, scn.absoluteSample, scn.ephs, sfs, scn.TOW)
    _same_plan(got, pc.plan(scn.settings, scn.status, scn.absoluteSample, scn.ephs, sfs, scn.TOW))
    assert got["n_meas"] == 0 and got["sampleEnd"] < got["sampleStart"]


def test_the_librarys_own_rules():
    scn = pc.host_cases()["b1c_5x7"]
    # an empty SatType drops the channel
    ephs = [dict(scn.ephs[0], SatType=0)] + scn.ephs[1:]
    got = native.pvt_plan(scn.settings, scn.status, scn.absoluteSample, ephs, scn.subFrameStart, scn.TOW)
    assert list(got["ready"]) == [pc.NO_SATTYPE, 1, 1, 1, 1] and got["n_meas"] > 0
    # no usable frame start / TOW drops it too
    for sfs, tow in [(np.inf, 7218.0), (0.0, 7218.0), (scn.n + 1.0, 7218.0), (3.0, np.inf)]:
        a, b = scn.subFrameStart.copy(), scn.TOW.copy()
        a[2], b[2] = sfs, tow
        assert native.pvt_plan(scn.settings, scn.status, scn.absoluteSample, scn.ephs, a, b)["ready"][2] == pc.NO_FRAME
    # absoluteSample must increase strictly on a ready channel ...
    bad = scn.absoluteSample.copy()
    bad[3, 20] = bad[3, 19]
    with pytest.raises(native.BdsError, match="strictly increasing"):
        native.pvt_plan(scn.settings, scn.status, bad, scn.ephs, scn.subFrameStart, scn.TOW)
    # ... and is not looked at on an idle one
    assert native.pvt_plan(scn.settings, "TTT-T", bad, scn.ephs, scn.subFrameStart, scn.TOW)["n_meas"] > 0


def test_solve_refuses_bad_arguments():
    scn = pc.host_cases()["b1c_4x1"]
    p, meas, _ = pc.run_reference(scn, n_meas=1)
    tt, sp, ck, _ = meas
    with pytest.raises(ValueError, match="satPos"):
        native.pvt_solve(scn.settings, scn.prns, p["ready"], p["sampleStart"], p["measSampleStep"], tt, sp[:, :3], ck)
    with pytest.raises(native.BdsError):
        native.pvt_solve(scn.settings.copy(c=0.0), scn.prns, p["ready"], p["sampleStart"], p["measSampleStep"], tt, sp, ck)
