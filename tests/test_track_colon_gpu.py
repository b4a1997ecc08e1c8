"""GPU parity of the tracking correlators on inputs where MATLAB's colon vector is NOT a + k d.

The replica index vectors of the reference are colon vectors tcode = a : d : b; MATLAB builds their second half from the right-hand
end point (csrc/bds_track.hip colon_vec / colon_at, oracle/matlab.py m_colon).  On every other record of this suite the two forms give
the same ceil() for every sample, so a device colon_at that returned a + k d throughout, took the wrong half at the junction or
mishandled the even mid-point would pass all of it.  tests/colon_states.py lists open-loop states on which thousands of samples sit on
a code-unit boundary and the two forms part by 3e-3 .. 1.2e-1 of |P| (its CPU guard is in tests/test_matlab_colon.py); here

  * the device correlators, open loop, against the float64 oracle (sample loop in C, colon form) on each of those states: run-based
    (SEG 8 and 16) and per-sample (default chunk and BDS_TRK_CHUNK=1024), every BDS_TRK_PREC the release documents.  All 18 sums
    within TOL[variant] of |P|; the same sums at least 100 x TOL from the oracle in its a + k d form (the test shows in its own
    output that it would have caught such a kernel), and TOL at least 100 x below the colon-vs-plain gap of the state;
  * closed-loop tracking from the natural start state (remCodePhase = 0, codeFreq = codeFreqBasis, acquiredFreq = IF: epoch 1 IS a
    row of the table) with the assertions of test_track_gpu.py::test_closed_loop_tracking, at 30.69 / 61.38 MS/s (B1C) and 102.3 MS/s
    (B2a), real and I/Q;
  * colon_at(colon_vec(a, d, b), k) itself, evaluated on the device by the test aid bds_track_colon, bit for bit against m_colon on
    the hand-worked cases of tests/test_matlab_colon.py -- which reach the branches the tracking path asserts away (n -= 1 after an
    overshoot, c snapped to b, c != b) -- and on every element of nine tracking vectors of the table.

Tolerances.  1e-6 of |P| is the suite's open-loop tolerance (tests/test_track_gpu.py): the default correlator (prec 4),
prec 5 and the per-sample kernel are held to it.  BDS_TRK_PREC 0-3 change the carrier and prefix-sum arithmetic, not the index, and
the project states no open-loop bound for them; theirs is 3 x the GPU-vs-oracle error measured on states of the same rates with the
code phase OFF the boundary lattice (colon_states.QUIET, eight states, 0 differing samples each; worst channel, all 18 sums, MI355X):
    prec 0 (fp32 carrier, fp32 prefix sums)                      2.61e-8 of |P|   -> 7.83e-8
    prec 1 (fp32 carrier, f64 prefix sums)                       2.28e-8          -> 6.84e-8
    prec 2 (f64 carrier recurrence)                              1.05e-10         -> 3.15e-10
    prec 3 (sin / cos of the reference's argument per sample)    8.51e-14         -> 2.55e-13
(on the same states: prec 4 8.5e-14, prec 5 8.5e-14, per-sample 2.5e-8.)  Every bound is at least 100 x below the smallest
colon-vs-plain gap of the table (3.1e-3); the test asserts that relation per state and channel.

Wide-band states use the reference's own dllCorrelatorSpacing (0.06 chip) or less: beyond 1 / 12 chip the early / late BOC(6,1)
indices leave [p(end) p p(1)] and MATLAB itself stops (colon_states.spacing_of); the C oracle used to read past its arrays there.
"""
import contextlib

import numpy as np
import pytest

import bds_amd
from oracle import cfast
from oracle.matlab import m_colon, m_colon_parts

import colon_states as cs
from helpers import assert_closed_loop_parity, track_case

pytestmark = pytest.mark.gpu

MEASURED = {0: 2.61e-8, 1: 2.28e-8, 2: 1.05e-10, 3: 8.51e-14}  # GPU-vs-oracle on colon_states.QUIET, of |P| (see the module docstring)
TOL = {4: 1e-6, 5: 1e-6, **{prec: 3 * m for prec, m in MEASURED.items()}}
# (variant, environment of the test-hooks build, BDS_TRK_PREC it runs with)
VARIANTS = [("runs", {}, 4), ("runs-seg8", {"BDS_TRK_SEG": "8"}, 4), ("runs-seg16", {"BDS_TRK_SEG": "16"}, 4),
            ("per-sample", {"BDS_TRK_PERSAMPLE": "1"}, 4), ("per-sample-chunk1024", {"BDS_TRK_PERSAMPLE": "1", "BDS_TRK_CHUNK": "1024"}, 4)]
VARIANTS += [(f"runs-prec{p}", {"BDS_TRK_PREC": str(p)}, p) for p in (0, 1, 2, 3, 5)]


@contextlib.contextmanager
def tuned(ctx, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx.reload_tuning()
    try:
        yield
    finally:
        for k in env:
            monkeypatch.delenv(k)
        ctx.reload_tuning()


@pytest.mark.parametrize("st", cs.STATES, ids=[s.name for s in cs.STATES])
def test_open_loop_against_the_oracle_on_colon_states(ctx, monkeypatch, st):
    s = cs.settings_of(st)
    x, chans = cs.record_of(st)
    ref = cs.oracle_sums(st, x, chans)
    plain = cs.oracle_sums(st, x, chans, plain=True)
    n = cs.n_sums(st)
    p = np.hypot(ref[:, 2], ref[:, 3])
    gap = np.abs(ref[:, :n] - plain[:, :n]).max(axis=1) / p  # oracle against oracle: what a + k d would cost on this state
    prn = [c.prn for c in chans]
    s6 = cs.state6_of(st, chans)
    print(f"\n{st.name}: blk {cs.blk_of(st)}, differing samples {cs.colon_counts(st)}, colon-vs-plain gap {gap[0]:.2e} / {gap[1]:.2e} of |P|")
    for name, env, prec in VARIANTS:
        tol = TOL[prec]
        with tuned(ctx, monkeypatch, env):
            got = ctx.track_correlate(s, x, prn, s6)
        for c in range(len(chans)):
            err = np.abs(got[c] - ref[c]).max() / p[c]
            far = np.abs(got[c, :n] - plain[c, :n]).max() / p[c]
            print(f"  {name:22s} ch {c}: {err:.2e} of |P| from the oracle, {far:.2e} from its a + k d form (tolerance {tol:.1e})")
            assert 100 * tol <= gap[c], (name, c)
            np.testing.assert_allclose(got[c], ref[c], rtol=0, atol=tol * p[c], err_msg=f"{name} ch {c}")
            assert far >= 100 * tol, (name, c)


# signal, mode, fs, IF, epochs, iq, further environments to repeat the run with
CLOSED = [("B1C", "WB", 30.69e6, 7.5e6, 10, False, [{"BDS_TRK_NBLOCKS": "2"}, {"BDS_TRK_PERSAMPLE": "1"}]),
          ("B1C", "NB", 30.69e6, 7.5e6, 8, False, []),
          ("B1C", "WB", 30.69e6, 7.5e6, 8, True, []),
          ("B1C", "WB", 61.38e6, 14.58e6, 8, False, []),
          ("B2A", "B2A", 102.3e6, 13.55e6, 40, False, [{"BDS_TRK_NBLOCKS": "2"}, {"BDS_TRK_PERSAMPLE": "1"}]),
          ("B2A", "B2A", 102.3e6, 13.55e6, 40, True, [])]


@pytest.mark.parametrize("signal,mode,fs,IF,n_epochs,iq,more", CLOSED,
                         ids=[f"{c[1]}-{c[2] / 1e6:g}{'-iq' if c[5] else ''}" for c in CLOSED])
def test_closed_loop_from_the_natural_start_state(ctx, monkeypatch, signal, mode, fs, IF, n_epochs, iq, more):
    cfast.build()
    spacing = cs.spacing_of(signal, mode)
    s, x, chans = track_case(signal, mode, n_epochs, iq=iq, fs=fs, IF=IF, zero_doppler=True, spacing=spacing)
    for ch in chans:
        assert ch.acquiredFreq == s.IF and ch.codeFreq == s.codeFreqBasis
    first = cs.State("epoch 1", signal, mode, fs, IF, iq, spacing, 0.0, None, None, True)
    assert max(cs.counts_read(first)) >= 100  # epoch 1 of every channel is an adversarial state
    ref = cfast.tracking_parallel(x, chans, s, mode=mode)
    lib = cs._trk_lib()
    lib.bds_oracle_trk_set_plain_colon(1)
    try:
        ref_plain = cfast.tracking_parallel(x, chans, s, mode=mode)
    finally:
        lib.bds_oracle_trk_set_plain_colon(0)
    with pytest.raises(AssertionError):  # oracle against oracle: the assertions below do tell the two forms apart on this record
        assert_closed_loop_parity(ref, ref_plain, mode)
    got, _ = bds_amd.tracking(x, chans, s, mode=mode)
    assert_closed_loop_parity(ref, got, mode)
    for env in more:
        with tuned(ctx, monkeypatch, env):
            got, _ = bds_amd.tracking(x, chans, s, mode=mode)
        assert_closed_loop_parity(ref, got, mode)


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.int64)


HAND = [(0.0, 0.1, 1.0),                                    # n = 10 even: mid-point (a + c) / 2, right half 1 - k 0.1
        (0.1, 0.1, 1.0),                                    # n = 9 odd: no mid-point, disjoint halves
        (0.3, 0.1, float(np.nextafter(0.3 + 7 * 0.1, 2.0))),  # a + n d one ulp short of b: c snapped to b
        (0.0, 0.3, 1.0),                                    # b well past a + n d: c = a + n d, NOT b
        (0.0, 0.3, 0.8),                                    # round() up, then the overshoot rule: n -= 1
        (-0.5, 1.0 / 15.0, 2.0), (0.25, 1.0 / 30.0, 7.0 + 1e-15)]


def test_device_colon_elements_bit_for_bit(ctx):
    """colon_at(colon_vec(a, d, b), k) on the device = m_colon(a, d, b)[k], the same 64 bits, with the same n and right-hand end"""
    for a, d, b in HAND:
        n, c = m_colon_parts(a, d, b)
        want = m_colon(a, d, b)
        val, c_dev, n_dev = ctx.track_colon(a, d, b, np.arange(n + 1))
        assert np.all(n_dev == n), (a, d, b, n, n_dev[0])
        assert np.all(_bits(c_dev) == _bits([c])), (a, d, b)
        np.testing.assert_array_equal(_bits(val), _bits(want), err_msg=f"{a}:{d}:{b}")
    differing = 0
    for name in ("b1c-wb-30.69-start", "b1c-wb-61.38-blk-1", "b2a-102.3-h-chunk-last-even"):
        st = next(s for s in cs.STATES if s.name == name)
        blk, step, sc = cs.blk_of(st), cs.step_of(st), (1.0 if st.signal == "B2A" else 2.0)
        for off in (-st.spacing, 0.0, st.spacing):  # E, P, L: tracking.m:260-286 / WB_tracking.m:289-317
            a, d, b = (st.rem + off) * sc, step * sc, (((blk - 1) * step + st.rem) + off) * sc
            want = m_colon(a, d, b)
            assert len(want) == blk
            val, c_dev, n_dev = ctx.track_colon(a, d, b, np.arange(blk))
            assert np.all(n_dev == blk - 1)
            assert np.all(_bits(c_dev) == _bits([m_colon_parts(a, d, b)[1]]))
            np.testing.assert_array_equal(_bits(val), _bits(want), err_msg=f"{name} offset {off}")
            differing += int(np.count_nonzero(want != a + np.arange(blk, dtype=np.float64) * d))
    assert differing > 100000  # these vectors are not a + k d: the comparison above bites
