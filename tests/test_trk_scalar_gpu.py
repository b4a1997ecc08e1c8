"""The per-epoch scalar stage of tracking on the device: the loop update (apply_update, through k_trk_update) and the C/N0 +
lock-detector post-pass (cno_pld_one, through k_trk_cno and k_trk_cno_seg), launched by the test aids bds_track_update and
bds_track_cno on the cases of tests/trk_scalar_cases.py (checked on the CPU by tests/test_trk_scalar_cases.py).

Order of every comparison: the NaN masks and each Inf mask of the device's output equal the reference's, and the reference's are
exactly what the case lists; then the finite values.
  * bit for bit against the float64 restatement of the .m files: what is formed by + - * / sqrt fmod alone (bds_track.hip is built
    with -ffp-contract=off) -- remCodePhase', remCarrPhase', dllDiscr, dllDiscrFilt, codeFreq', the QMBOC composites, the stored
    state and sums, the lock detector
  * against the 50-digit value: what lies behind atan, log10 or the complex branch -- pllDiscr, pllDiscrFilt, carrFreq' and the
    carrier filter's state (relative to the output's scale, trk_scalar_cases.update_mp), and C/N0 (in dB).  The bound is 4 x the
    worst error measured on an MI355X (MEASURED below; every test prints its figures, profiles/trk_scalar_errors.txt keeps them);
    a measured error above 1e-13 (1e-9 dB) would be a finding, not a bound.
(`lin` itself is not among the outputs of the post-pass: on the d > 0 branch it is seen through 10 log10.)

End to end, small: a channel moved to a PRN that is not in the record takes the complex branch in the library's own runs, one-shot
and in pieces, against the oracle; and a record that turns to zeros stops its channel at the non-finite code NCO."""
import numpy as np
import pytest

import bds_amd

from helpers import assert_closed_loop_parity
from test_track_session_gpu import joined, run_session
from track_session_cases import PIECES

import trk_scalar_cases as tc

pytestmark = pytest.mark.gpu

# worst errors measured on an MI355X (gfx950, ROCm 7.0.2) over all cases (profiles/trk_scalar_errors.txt): C/N0 in dB against the
# 50-digit value -- the worst is an interval of noise-m50-pm2 near d = 0, where the float64 restatement is off by the same amount: the
# device is bit-equal to it there --; the update's outputs against the unrounded 50-digit value, relative to their scale (eps is 2.2e-16)
MEASURED = {"cno_db": 7.851e-13, "pllDiscr": 1.415e-16, "pllDiscrFilt": 1.566e-16, "carrFreq'": 6.62e-17, "d2CarrError'": 5.686e-17,
            "dCarrError'": 1.229e-16}
FINDING = {"cno_db": 1e-9, "update": 1e-13}  # the budgets bench.py and the f64 decision tests state

CNO_NAMES = [c.name for c in tc.cno_cases()]
UPD_NAMES = [c.name for c in tc.update_cfgs()]
CNO_ROWS = {0: (0,), 1: (0, 2, 4), 2: (0, 2, 4)}
PLD_ROWS = {0: (1,), 1: (1, 3), 2: (1, 3)}


def assert_masks(got, ref, want, what):
    """NaN and +-Inf by position: the device against the reference, the reference against what the case lists"""
    for kind, g, r, w in zip(("nan", "+inf", "-inf"), (np.isnan(got), got == np.inf, got == -np.inf),
                             (np.isnan(ref), ref == np.inf, ref == -np.inf), want):
        assert np.array_equal(r, w), (what, kind, "reference")
        assert np.array_equal(g, r), (what, kind)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def one_shot(ctx, case):
    return ctx.track_cno(tc.cno_settings(case), case.prompts, case.done, tc.n_cno_of(case))


# ---- C/N0 and lock detector -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CNO_NAMES)
def test_cno_post_pass(ctx, name):
    case = tc.cno_case(name)
    got = one_shot(ctx, case)
    f64, _ = tc.cno_f64(name)
    ref, _ = tc.cno_mp(name)
    want = tc.cno_expected_masks(case)
    assert_masks(got, ref, want, name)
    assert_masks(got, f64, want, name)
    fin = np.isfinite(ref)
    rows, pld = list(CNO_ROWS[case.pm]), list(PLD_ROWS[case.pm])
    assert np.array_equal(got[pld][fin[pld]], f64[pld][fin[pld]])  # the lock detector: bit for bit
    unused = [r for r in range(5) if r not in rows + pld]
    assert np.all(got[unused] == 0)
    err = np.abs(got[rows][fin[rows]] - ref[rows][fin[rows]])
    print(f"trk_scalar_error: cno {name}: {err.size} values, worst {err.max():.3e} dB")
    assert err.max() <= FINDING["cno_db"], "a finding: above the 1e-9 dB budget"
    assert err.max() <= 4 * MEASURED["cno_db"]


@pytest.mark.parametrize("name", CNO_NAMES)
def test_cno_in_pieces_is_the_one_shot_result(ctx, name):
    case = tc.cno_case(name)
    want = one_shot(ctx, case)
    for pieces in tc.piece_lists(case.prompts.shape[2], case.M):
        got = ctx.track_cno(tc.cno_settings(case), case.prompts, case.done, tc.n_cno_of(case), pieces=pieces)
        assert same_bits(got, want), pieces[:6]


# ---- the loop update ------------------------------------------------------------------------------------------------
def run_update(ctx, cfg):
    new, active, completed, out = ctx.track_update(cfg.settings, np.array([r.state for r in cfg.rows]), np.array([r.sums for r in cfg.rows]))
    res = []
    for i in range(len(cfg.rows)):
        d = {f: float(out[f][i]) for f in tc.EPOCH_FIELDS}
        d.update({f: float(new[i, j]) for j, f in enumerate(tc.NEXT)})
        d["active'"], d["completed'"] = int(active[i]), int(completed[i])
        res.append(d)
    return res


@pytest.mark.parametrize("name", UPD_NAMES)
def test_loop_update(ctx, name):
    cfg = tc.update_cfg(name)
    worst = {k: 0.0 for k in tc.MP_UPDATE}
    for row, got in zip(cfg.rows, run_update(ctx, cfg)):
        f64 = tc.update_f64(cfg, row)
        val, scale, raw = tc.update_mp(cfg, row)
        what = (name, row.name)
        # NaN and Inf by position, before any value: the device's, the restatement's, and what the row lists
        assert {k for k, v in f64.items() if np.isnan(v)} == set(row.nan), what
        assert {k for k, v in got.items() if np.isnan(v)} == set(row.nan), what
        assert not any(np.isinf(v) for v in f64.values()) and not any(np.isinf(v) for v in got.values()), what
        assert got["active'"] == f64["active'"] == (0 if row.stop else 1), what
        assert got["completed'"] == 1, what
        for k in tc.EXACT_UPDATE:
            if k in row.nan:
                continue
            assert got[k] == f64[k] and np.signbit(got[k]) == np.signbit(f64[k]), (what, k, got[k], f64[k])
        for k in tc.MP_UPDATE:
            if k in row.nan:
                continue
            worst[k] = max(worst[k], tc.update_error(k, got[k], raw[k], scale[k]))
    for k, e in worst.items():
        print(f"trk_scalar_error: update {name}: {k} worst {e:.3e} of its scale")
        assert e <= FINDING["update"], (k, "a finding: above the 1e-13 budget")
        assert e <= 4 * MEASURED[k], k


@pytest.mark.parametrize("name", ["b2a-pilot", "nb-data", "wb-pilot"])
def test_zero_sums_stop_the_channel(ctx, name):
    """an epoch of all-zero samples: atan(0/0), 0/0 in the DLL.  The epoch's outputs are stored as computed, the channel stops as at a
    short read, and its neighbours in the launch go on"""
    cfg = tc.update_cfg(name)
    res = dict(zip((r.name for r in cfg.rows), run_update(ctx, cfg)))
    z = res["zero-sums"]
    assert z["active'"] == 0 and z["completed'"] == 1
    assert all(np.isnan(z[f]) for f in ("pllDiscr", "pllDiscrFilt", "dllDiscr", "dllDiscrFilt", "codeFreq'", "carrFreq'"))
    assert z["I_P"] == 0 and z["Q_P"] == 0 and np.isfinite(z["remCodePhase'"]) and np.isfinite(z["codeFreq"])
    assert res["typical"]["active'"] == 1 and res["pll-0/0"]["active'"] == 1
    assert res["codefreq<=0"]["active'"] == 0 and res["codefreq<=0"]["codeFreq'"] < 0


# ---- end to end -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["b2a", "b1c-wb"])
def test_a_channel_without_its_satellite(ctx, which):
    s, x, chans, mode = tc.e2e_case(which)
    chans = list(chans)
    ref = tc.e2e_oracle(which)
    sig = "B2a_CNo" if mode == "B2A" else "B1C_CNo"
    got, _ = bds_amd.tracking(x, chans, s, mode=mode)
    n = len(got[0].I_P)
    calls, _ = run_session(x, chans, s, PIECES[n][0], mode=mode)
    for res in (got, joined(calls, got)):
        for r in res:
            assert r.completed == n
            for f in ("DataCNo", "PilotCNo", sig):
                assert np.all(np.isfinite(getattr(r, f))), f
        assert_closed_loop_parity(ref, res, mode)


def test_a_record_that_turns_to_zeros(ctx):
    s, x, chans = tc.zero_stretch_case()
    chans = list(chans)
    from oracle import tracking as otrk

    ref, _ = otrk.tracking(otrk.RawFile(x), chans, s, mode="B2A")
    got, _ = bds_amd.tracking(x, chans, s)
    assert [g.completed for g in got] == [3, 0, 0] and [g.status for g in got] == ["-"] * 3
    g, r = got[0], ref[0]
    np.testing.assert_array_equal(g.absoluteSample, r.absoluteSample)
    p = np.hypot(r.I_P, r.Q_P).max()
    tol = dict(codeFreq=1e-6, carrFreq=1e-3, dllDiscr=1e-6, dllDiscrFilt=1e-6, pllDiscr=1e-6, pllDiscrFilt=1e-3, remCodePhase=1e-7,
               remCarrPhase=1e-6, DataCNo=1e-3, PilotCNo=1e-3, B2a_CNo=1e-3)  # helpers.assert_closed_loop_parity's
    tol.update({f: 1e-4 * p for f in ("I_E", "I_P", "I_L", "Q_E", "Q_P", "Q_L", "Pilot_I_P", "Pilot_Q_P")})
    for f, atol in tol.items():
        a, b = getattr(g, f), getattr(r, f)
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a == np.inf, b == np.inf), f  # NaN and the template's Inf
        fin = np.isfinite(b)
        np.testing.assert_allclose(a[fin], b[fin], rtol=0, atol=atol, err_msg=f)
    assert np.isnan(g.pllDiscr[2]) and np.isnan(g.dllDiscr[2]) and g.I_P[2] == 0 and g.Q_P[2] == 0
    assert np.all(np.isinf(g.pllDiscr[3:])) and np.all(g.absoluteSample[3:] == 0)
    for later in got[1:]:
        assert np.all(np.isinf(later.remCodePhase)) and np.all(later.absoluteSample == 0)
