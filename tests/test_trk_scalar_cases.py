"""The cases of tests/trk_scalar_cases.py are what tests/test_trk_scalar_gpu.py takes them for -- checked on the CPU, before a GPU
sees them: the float64 restatement of the .m files lies within its conditioning bound of the 50-digit evaluation of the same
expressions, its NaN and Inf sit exactly where the cases list them, and every case has the property it is named for."""
import numpy as np
import pytest

from oracle import tracking as otrk

import trk_scalar_cases as tc

CNO_NAMES = [c.name for c in tc.cno_cases()]
UPD_NAMES = [c.name for c in tc.update_cfgs()]
CNO_ROWS = {0: (0,), 1: (0, 2, 4), 2: (0, 2, 4)}  # the C/N0 rows of cno5 a pilot mode writes


def masks(a):
    return np.isnan(a), a == np.inf, a == -np.inf


def test_cases_cover_what_the_kernels_branch_on():
    cases = tc.cno_cases()
    assert {c.M for c in cases} == {2, 3, 5, 10, 50, 200}
    assert {c.pm for c in cases} == {0, 1, 2}
    assert {c.prompts.shape[1] for c in cases} == {1, 2, 3}
    assert max(tc.n_cno_of(c) for c in cases) == 257  # more intervals than the workgroup has threads
    assert {c.prop for c in cases} == {"d>0", "noise", "second-interval", "special", "pld", "done"}
    cfgs = tc.update_cfgs()
    assert {(c.mode, c.pilot) for c in cfgs} >= {("B2A", True), ("B2A", False), ("NB", True), ("NB", False), ("WB", True)}
    assert sum(c.name.startswith("colon-") for c in cfgs) >= 25


# ---- C/N0 and lock detector -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CNO_NAMES)
def test_cno_restatement_within_its_bound_of_50_digits(name):
    case = tc.cno_case(name)
    f64, _ = tc.cno_f64(name)
    ref, bound = tc.cno_mp(name)
    want = tc.cno_expected_masks(case)
    for got_m, ref_m, want_m, what in zip(masks(f64), masks(ref), want, ("nan", "+inf", "-inf")):
        assert np.array_equal(ref_m, want_m), what  # the reference holds NaN / Inf exactly where the case lists them
        assert np.array_equal(got_m, want_m), what
    fin = np.isfinite(ref)
    assert np.all(np.abs(f64[fin] - ref[fin]) <= bound[fin])
    rows = list(CNO_ROWS[case.pm])
    assert bound[rows].max() < tc.COND_MAX_DB  # no interval so close to d = 0 that its own rounding reaches the budget
    if not case.kinds:
        assert fin.all()  # a finite case holds neither NaN nor Inf


@pytest.mark.parametrize("name", CNO_NAMES)
def test_cno_case_has_its_property(name):
    case = tc.cno_case(name)
    f64, d = tc.cno_f64(name)
    streams = 2 if case.pm else 1
    M, T = case.M, tc.cno_settings(case).intTime
    ev = ~np.isnan(d[:streams])  # intervals that were evaluated
    if case.prop == "d>0":
        assert ev.all() and np.all(d[:streams] > 0)
    elif case.prop == "noise":
        assert ev.all()
        assert np.mean(d[0] < 0) >= 1 / 3  # the data prompts alone
        assert all(np.any(d[st] < 0) for st in range(streams))  # (and some of the pilot's)
        assert np.any(d[:streams] > 0)
    elif case.prop == "second-interval":
        assert tc.n_cno_of(case) == 257 and case.prompts.shape[1] == 1
        assert d[0, 0, 256] < 0 and d[1, 0, 256] < 0  # thread 0's second interval takes the complex branch
        assert np.any(d[:, 0, :256] > 0) and np.any(d[:, 0, :256] < 0)
    elif case.prop == "special":
        assert set(case.kinds.values()) == {"nan", "+inf", "-inf"}
        assert {k[0] for k in case.kinds} == {0, 1}  # in the data stream and in the pilot stream
        for (stream, ch, q), kind in case.kinds.items():
            i, qq = tc._streams(case, ch, q)[stream]
            dd, lin, cno, pld = tc.cno_one_f64(i, qq, M, T)
            if kind == "-inf":
                assert dd == 0.0 and lin == 0.0 and cno == -np.inf and pld == 1.0  # Zm = 21, Zv = 441
            elif kind == "+inf":
                assert dd == 625.0 and lin == np.inf and cno == np.inf and np.isfinite(pld)  # Zv = 0: Nv = 0
            else:
                assert np.isnan(cno) and np.isnan(pld)
        # the smoothing passes each of them on to the next interval, and adds -Inf and +Inf to NaN
        nan, pinf, ninf = tc.cno_expected_masks(case)
        assert nan[0, 0].tolist() == [False, False, False, True, True, False, True, False, False]
        assert pinf[0, 0].tolist() == [False, True, True, False, False, False, False, True, False]
        assert ninf[0, 0].tolist() == [False, False, False, False, False, True, False, False, False]
        assert np.array_equal(nan[2, 1], nan[0, 0]) and np.array_equal(pinf[2, 1], pinf[0, 0]) and np.array_equal(ninf[2, 1], ninf[0, 0])
        assert not nan[0, 1].any() and not pinf[0, 1].any()  # the other stream of either channel stays finite
    elif case.prop == "pld":
        p = case.prompts
        assert np.all(p[0, 0, :5] > 0) and np.all(p[0, 0, 5:] < 0) and p[1, 0, :5].sum() == 0 and p[1, 0, 5:].sum() == 0
        assert np.all(p[0, 1] == 0) and p[1, 1, :5].sum() != 0 and p[1, 1, 5:].sum() != 0
        assert np.any(p[0, 2] == 0) and np.any(p[0, 2] > 0) and np.any(p[0, 2] < 0)
        assert f64[1, 0].tolist() == [1.0, 1.0] and f64[1, 1].tolist() == [-1.0, -1.0]
        assert np.all(np.abs(f64[1, 2]) < 1)
    elif case.prop == "done":
        assert case.done[0] == case.prompts.shape[2] and case.done[1] % M and 0 < case.done[2] < M
        nd = case.done // M
        for ch in range(3):
            assert np.all(f64[:, ch, nd[ch]:] == 0) and np.all(f64[0, ch, :nd[ch]] != 0)


@pytest.mark.parametrize("name", CNO_NAMES)
def test_piece_lists_cross_every_interval_boundary(name):
    case = tc.cno_case(name)
    n, M = case.prompts.shape[2], case.M
    inside, mixed = tc.piece_lists(n, M)
    for pieces in (inside, mixed):
        assert sum(pieces) == n and min(pieces) >= 1
    edges = set(np.cumsum(inside)[:-1].tolist())
    assert not any(b in edges for b in range(M, n, M))  # every boundary lies strictly inside a piece
    edges = set(np.cumsum(mixed)[:-1].tolist())
    assert 1 in mixed and any(b in edges for b in range(M, n, M))  # ... and here a call ends ON a boundary


def test_oracle_cno_takes_the_complex_branch():
    """oracle.tracking.calc_cno_pld (pairwise sums, not the kernel's order) on the noise intervals: finite, and the 50-digit value"""
    case = tc.cno_case("noise-m10-pm0")
    s = tc.cno_settings(case)
    _, d = tc.cno_f64(case.name)
    n = 0
    for q in np.flatnonzero(d[0, 0] < 0):
        sl = slice(q * case.M, (q + 1) * case.M)
        cno, pld = otrk.calc_cno_pld(case.prompts[0, 0, sl], case.prompts[1, 0, sl], None, None, s, 0)
        ref = tc.cno_one_mp(case.prompts[0, 0, sl], case.prompts[1, 0, sl], case.M, s.intTime)
        assert np.isfinite(cno[0]) and abs(cno[0] - float(ref["cno"])) <= tc.DB * float(ref["rel"]) + 4 * tc.EPS * abs(cno[0])
        n += 1
    assert n >= 3


# ---- the loop update ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", UPD_NAMES)
def test_update_restatement_within_its_bound_of_50_digits(name):
    cfg = tc.update_cfg(name)
    for row in cfg.rows:
        f64 = tc.update_f64(cfg, row)
        val, scale, raw = tc.update_mp(cfg, row)
        nan = {k for k, v in f64.items() if np.isnan(v)}
        assert nan == set(row.nan), (row.name, nan)  # NaN exactly where the row lists it
        assert not any(np.isinf(v) for v in f64.values()), row.name
        assert f64["active'"] == (0 if row.stop else 1) and f64["completed'"] == 1, row.name
        for k, ref in val.items():
            if k in row.nan:
                assert np.isnan(ref), (row.name, k)
                continue
            assert tc.update_error(k, f64[k], raw[k], scale[k]) <= tc.UPDATE_OPS * tc.EPS, (row.name, k, f64[k], ref)


@pytest.mark.parametrize("name", ["b2a-pilot", "b2a-data", "nb-pilot", "nb-data", "wb-pilot"])
def test_update_rows_have_their_property(name):
    cfg = tc.update_cfg(name)
    rows = {r.name: r for r in cfg.rows}
    out = {r.name: tc.update_f64(cfg, r) for r in cfg.rows}
    two_pi = 2 * np.pi

    def data_atan(n):  # the data discriminator alone, from the row's sums
        i, q = 0.0 + rows[n].sums[2], rows[n].sums[3]
        with np.errstate(all="ignore"):
            return float(np.arctan(np.float64(q) / np.float64(i)) / two_pi)

    assert data_atan("ip+0-q+") == data_atan("ip-0-q+") == 0.25 and data_atan("ip+0-q-") == data_atan("ip-0-q-") == -0.25
    assert np.signbit(rows["ip-0-q+"].sums[2]) and not np.signbit(rows["ip+0-q+"].sums[2])
    for n in ("ip+0-q+", "ip-0-q+", "ip+0-q-", "ip-0-q-"):
        assert np.isfinite(out[n]["pllDiscr"]) and out[n]["active'"] == 1
    assert out["ip+0-q+"]["pllDiscr"] == out["ip-0-q+"]["pllDiscr"] != out["ip+0-q-"]["pllDiscr"]
    # atan, not atan2: I_P < 0 with Q_P > 0 is a small NEGATIVE angle, where atan2 gives almost half a cycle
    r = rows["ip-neg"]
    assert r.sums[2] < 0 < r.sums[3] and -0.05 < data_atan("ip-neg") < 0 < np.arctan2(r.sums[3], r.sums[2]) / two_pi
    assert out["e=l"]["dllDiscr"] == 0.0 and out["typical"]["dllDiscr"] != 0.0
    assert out["codefreq<=0"]["codeFreq'"] < 0 and np.isfinite(out["codefreq<=0"]["codeFreq'"]) and out["codefreq<=0"]["active'"] == 0
    assert out["trig-negative"]["remCarrPhase'"] < 0  # rem() keeps the sign of trigarg
    assert abs(rows["trig-large"].state[2]) * two_pi * 1e-3 > 1e6 and 0 <= out["trig-large"]["remCarrPhase'"] < two_pi
    assert out["rem-negative"]["remCodePhase"] < 0
    assert out["zero-sums"]["active'"] == 0 and out["e+l=0"]["active'"] == 0 and out["pll-0/0"]["active'"] == 1
    if cfg.pilot:
        r = rows["pilot-denominator-0"]
        assert r.sums[9] == 0 and r.sums[14] == 0 and np.isfinite(out[r.name]["pllDiscr"])
        if cfg.mode == "B2A":
            rot = np.exp(-1j * np.pi / 2)
            assert rot.real == 6.123233995736766e-17 and rot.imag == -1.0  # cos(-pi/2) as float64 arithmetic gives it
            re = r.sums[8] * rot.real - r.sums[9] * rot.imag
            assert re != 0 and abs(re) < 1e-10  # a finite quotient, where an exact rotation divides by zero
            # ... whose angle is within 1e-16 of the exact rotation's -+ 1/4 cycle
            assert abs(abs(2 * out[r.name]["pllDiscr"] - data_atan(r.name)) - 0.25) < 1e-15
    else:
        assert all(out["typical"][f] == 0.0 for f in ("Pilot_I_P", "Pilot_Q_P", "Pilot_I_E"))
    if cfg.mode == "WB":
        assert out["typical"]["Pilot_I_E"] != 0.0 and out["typical"]["Pilot_I_P"] != rows["typical"].sums[8]  # the composite, not the sum


def test_code_phase_update_equals_the_colon_vectors_end():
    """the update forms remCodePhase' from rem + (blk - 1) step, the correlators index with the colon vector, whose
    last element is its end point c.  On every state of tests/colon_states.py (at the block tracking takes) and on 4000 random code
    NCO states the two are the same float64 number, and the colon vector has blk elements."""
    n = 0
    for cfg in tc.update_cfgs():
        if not cfg.name.startswith("colon-"):
            continue
        (row,) = cfg.rows
        tp_last, blk, step = tc.tp_last_of(cfg, row)
        rem = float(row.state[1])
        kernel = rem + (blk - 1) * step if cfg.mode == "B2A" else rem * 2.0 + (blk - 1) * (step * 2.0)
        assert kernel == tp_last, cfg.name
        n += 1
    assert n >= 25
    assert tc.colon_scan() == (0, 0)


# ---- end to end -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["b2a", "b1c-wb"])
def test_end_to_end_case_takes_the_complex_branch_in_the_oracles_own_run(which):
    s, _, chans, mode = tc.e2e_case(which)
    assert chans[-1].PRN == tc.ABSENT_PRN and all(c.PRN != tc.ABSENT_PRN for c in chans[:-1])
    assert tc.e2e_negative_intervals(which) >= tc.E2E_MIN_NEGATIVE[which]
    for r in tc.e2e_oracle(which):
        assert r.status == "T"
        for f in ("DataCNo", "PilotCNo", "B2a_CNo" if mode == "B2A" else "B1C_CNo"):
            assert np.all(np.isfinite(getattr(r, f))), f  # (NaN before the complex branch was restated)


def test_oracle_stops_at_a_non_finite_code_nco():
    s, x, chans = tc.zero_stretch_case()
    ref, _ = otrk.tracking(otrk.RawFile(x), list(chans), s, mode="B2A")
    r = ref[0]
    assert r.status == "-"
    assert np.isfinite(r.remCodePhase).sum() == 3  # three epochs stored, the third with its NaN discriminators
    assert np.all(x[int(r.absoluteSample[2]):] == 0) and r.I_P[2] == 0 and r.Q_P[2] == 0
    assert np.isnan(r.pllDiscr[2]) and np.isnan(r.dllDiscr[2]) and np.isfinite(r.pllDiscr[:2]).all()
    assert np.all(np.isinf(r.pllDiscr[3:])) and np.all(r.absoluteSample[3:] == 0)  # the template: no fourth epoch was begun
    assert np.isfinite(r.DataCNo[0]) and np.all(r.DataCNo[1:] == 0)
    for later in ref[1:]:  # as at a short read, later channels are never started
        assert later.status == "-" and np.all(np.isinf(later.remCodePhase))
