"""The restatement of tests/pvt_cases.py itself (CPU): its constants against the reference's own literals
(tests/golden/pvt_constants.json), its fix against the true receiver position of a built scenario, and each deliberate change of
`Model` rejected -- so that what the library is compared with is known to be right.

The closed-loop bound, a condition on the INPUTS which the restatement alone must meet:
    |fix - truth| <= ||pinv(A)||_2 sqrt(n_sat) (2 ulp(TOW) c + 1e-4 m)
A is the restatement's final matrix; 2 ulp(TOW) c is the rounding of seconds-of-week in f64 (about 8.7 mm per ulp below 2^18 s),
1e-4 m the range acceleration ignored within one code period.
"""
import json
import os
import re
from dataclasses import replace

import numpy as np
import pytest

import bds_amd
import pvt_cases as pc
from bds_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_LIGHT = 299792458.0
GATE_MS = bds_amd.pvt.RECORD_GATE_MS  # (the restatement is test infrastructure of the position fix: without the feature, no test here)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "pvt_constants.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def scn_b1c():
    return pc.make_scenario("B1C", 5, 120, overrides=dict(useTropCorr=0, navSolPeriod=100))


def _err(scn, sol):
    return np.sqrt((sol["X"] - scn.rx[0]) ** 2 + (sol["Y"] - scn.rx[1]) ** 2 + (sol["Z"] - scn.rx[2]) ** 2)


def _bounds(scn, sol):
    return np.array([pc.truth_bound(A, scn.tow, C_LIGHT) for A in sol["A"]])


def test_constants_are_the_references(golden):
    g = golden
    assert (pc.BDS_PI, pc.OMEGA_E, pc.MU, pc.F_REL) == (float(g["bdsPi"]), float(g["OmegaE"]), float(g["mu"]), float(g["F"]))
    assert (pc.A_REF_MEO, pc.A_REF_IGSO_GEO, pc.HALF_WEEK) == (int(g["A_ref_MEO"]), int(g["A_ref_IGSO_GEO"]), int(g["half_week"]))
    assert pc.OMEGAE_DOT == float(g["Omegae_dot"])
    assert (pc.ELL5_A, pc.ELL5_FINV) == (int(g["ellipsoid5_a"]), float(g["ellipsoid5_finv"]))
    assert (pc.TOPO_A, pc.TOPO_FINV) == (float(g["topocent_a"]), float(g["topocent_finv"]))
    assert pc.TROPO == {"a_e": float(g["tropo_a_e"]), "b0": float(g["tropo_b0"]), "tlapse": float(g["tropo_tlapse"])}
    assert pc.TROPO_ARGS == tuple(float(v) for v in g["tropo_args"])
    assert (int(g["iterations"]), int(g["first_trop"])) == (10, 2)


def test_library_sources_and_settings_carry_the_same_constants(golden):
    g = golden
    csrc = os.path.join(ROOT, "bds-3-b1c-b2a-sdr-receiver_amd", "csrc")
    dev = open(os.path.join(csrc, "bds_pvt_math.h")).read()
    host = open(os.path.join(csrc, "bds_pvt.cpp")).read()
    for name in ("bdsPi", "OmegaE", "mu", "F", "A_ref_MEO", "A_ref_IGSO_GEO", "half_week"):
        assert re.search(r"[ (=]" + re.escape(g[name]) + r"\b", dev), name
    for name in ("Omegae_dot", "ellipsoid5_a", "ellipsoid5_finv", "topocent_a", "topocent_finv", "tropo_a_e", "tropo_b0", "tropo_tlapse"):
        assert re.search(r"[ (=]" + re.escape(g[name]) + r"\b", host), name
    for sig, init in (("B1C", bds_amd.init_settings_b1c), ("B2A", bds_amd.init_settings_b2a)):
        s = init()
        for name in native.PVT_SETTINGS:
            assert getattr(s, name) == float(g[sig][name]), (sig, name)
        assert GATE_MS[sig] == int(g[sig]["gate_ms"])


def test_pack_pvt_params_names_a_missing_setting():
    s = bds_amd.init_settings_b1c()
    for name in native.PVT_SETTINGS:
        t = s.copy()
        delattr(t, name)
        with pytest.raises(AttributeError, match=name):
            native.pack_pvt_params(t)


def test_header_declares_the_entries_and_the_python_layer_binds_them():
    src = open(os.path.join(ROOT, "include", "bds_mi355x.h")).read()
    for entry in ("bds_pvt_plan", "bds_pvt_measure", "bds_pvt_solve", "bds_post_navigation"):
        assert re.search(r"BDS_API\s+int\s+%s\s*\(" % entry, src) and entry in native.EXPORTS and hasattr(native.lib(), entry)
    for name in ("post_navigation", "postNavigation", "pvt_plan", "pvt_measure", "pvt_solve"):
        assert hasattr(bds_amd, name)
    assert hasattr(native.Context, "pvt_measure") and hasattr(native.Context, "post_navigation")


@pytest.mark.parametrize("signal,n,period", [("B1C", 120, 100), ("B2A", 1300, 100)])
def test_closed_loop_meets_the_bound(signal, n, period):
    scn = pc.make_scenario(signal, 6, n, overrides=dict(useTropCorr=0, navSolPeriod=period), seed=3)
    assert scn.tow < 262144 and len(set(scn.subFrameStart)) > 1
    p, meas, sol = pc.run_reference(scn)
    assert p["n_meas"] >= 5 and all(len(a) == 6 for a in sol["active"])
    err, bound = _err(scn, sol), _bounds(scn, sol)
    print("closed loop", signal, "worst error / bound [m]", err.max(), bound.min())
    assert (err <= bound).all()
    # the clock: forced to 0 at the first fix; afterwards localTime is corrected, and the receiver clock of the scenario does not drift
    assert sol["dt"][0] == 0 and (np.abs(sol["dt"][1:]) <= bound[1:]).all()
    lat, lon, h = pc.cart2geo5(*scn.rx)
    np.testing.assert_allclose([sol["latitude"][0], sol["longitude"][0]], [lat, lon], atol=1e-7)
    assert abs(sol["height"][0] - h) <= bound[0]


@pytest.mark.parametrize("change", [dict(e_r_corr=False), dict(tgd_sign=1.0), dict(sfs_offset=1), dict(dt1_zero=False)])
def test_deliberate_changes_miss_the_bound(scn_b1c, change):
    _, _, good = pc.run_reference(scn_b1c, n_meas=3)
    assert (_err(scn_b1c, good) <= _bounds(scn_b1c, good)).all() and good["dt"][0] == 0
    _, _, bad = pc.run_reference(scn_b1c, replace(pc.REFERENCE, **change), n_meas=3)
    if "dt1_zero" in change:
        assert abs(bad["dt"][0]) > 1e3  # the first guess of the local time is tens of microseconds off at the very least
    else:
        assert (_err(scn_b1c, bad) > 10 * _bounds(scn_b1c, bad)).all()


def test_check_t_matters_across_the_week_boundary():
    # t_oe, t_oc = 604500 s, TOW = 108 s: time - t_oe = -604392 s, which check_t.m:25-26 turns into 408 s
    scn = pc.make_scenario("B1C", 5, 60, tow=108, t_oe=604500, overrides=dict(useTropCorr=0, navSolPeriod=100), seed=5)
    _, _, good = pc.run_reference(scn)
    assert (_err(scn, good) <= _bounds(scn, good)).all()
    _, _, bad = pc.run_reference(scn, replace(pc.REFERENCE, check_t=False))
    assert (_err(scn, bad) > 1e3).all()


def test_index_search_is_the_references_scan(scn_b1c):
    """The two changes of the index search move no position (the code phase is continuous across an interval's end, so the
    neighbouring interval extrapolates to the same transmit time within the bound): they are caught against the loop of
    calculatePseudoranges.m:76-82 as written -- also at a sample EQUAL to an entry, and past the last entry."""
    a = scn_b1c.absoluteSample[1]
    n = len(a)
    samples = np.array([a[3] + 1, a[7], a[7] - 1, a[n - 2], a[n - 1] - 1, a[n - 1], a[n - 1] + 5e6, (a[10] + a[11]) / 2])
    want = np.array([pc.index_scan(a, s) for s in samples])
    assert want[1] == 8 and want[2] == 7 and want[4] == n - 1 and want[5] == n - 1 and want[6] == n - 1
    np.testing.assert_array_equal(pc.index_search(a, samples), want)
    assert (pc.index_search(a, samples, replace(pc.REFERENCE, index_ge=True)) != want).any()
    assert (pc.index_search(a, samples, replace(pc.REFERENCE, index_minus1=False)) != want).all()
    # the scan with the reference's running start (searchIndex) gives the same as from 1
    start = 1
    for s in np.sort(samples):
        k = pc.index_scan(a, s, start)
        assert k == pc.index_scan(a, s)
        start = k + 1


def test_satpos_agrees_with_extended_precision(scn_b1c):
    """f64 against the same formulas in longdouble: the restatement's own rounding, which the 1e-6 m tolerance of the device test
    has to cover (~1 ulp errors of sin, cos and atan2 reach E and u as ~3e-15 rad, times 4.2e7 m ~ 1.3e-7 m; 8x margin)."""
    t = scn_b1c.tow + np.linspace(-0.1, 1.1, 50)
    worst = 0.0
    for e in scn_b1c.ephs:
        p64, c64 = pc.satpos(t, e, True)
        pl, cl = pc.satpos(t, e, True, dtype=np.longdouble)
        worst = max(worst, float(np.abs(p64 - pl).max()))
        assert float(np.abs(c64 - cl).max()) < 1e-18
    print("satpos f64 - longdouble, worst [m]", worst)
    assert worst < 1e-6


def test_rank_rule_and_degenerate_geometry():
    A = np.array([[0.1, 0.2, 0.97, 1], [0.5, -0.3, 0.81, 1], [0.1, 0.2, 0.97, 1], [-0.4, 0.6, 0.69, 1.0]])
    assert pc.matlab_rank(A) == 3 and pc.matlab_rank(np.eye(4)) == 4 and pc.matlab_rank(np.full((4, 4), np.nan)) == 0
    assert pc.cart2geo5(0, 0, 0)[1] == 0 and np.isnan(pc.cart2geo5(0, 0, 0)[0]) and np.isnan(pc.cart2geo5(0, 0, 0)[2])
