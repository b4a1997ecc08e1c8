"""The float64 model of the correlation function (tests/corrfn_cases.py) and bds_amd.track_states, without a GPU: at the trackers'
own taps the model reproduces the oracle's correlator sums; track_states rebuilds the oracle's per-epoch NCO states exactly; the
model has the shape of the code's autocorrelation; and models with one deliberate change of the index rule each are told apart
from it by more than the tolerance the GPU test holds the kernel to."""
import functools
import os
import re

import numpy as np
import pytest

import bds_amd
from bds_amd import native, synth
from oracle import tracking as otrk

import corrfn_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("B2A", "B2A", 4, False), ("B1C", "NB", 3, False), ("B1C", "WB", 3, False),
         ("B2A", "B2A", 4, True), ("B1C", "NB", 3, True), ("B1C", "WB", 3, True)]


@functools.lru_cache(maxsize=None)
def traced(signal, mode, n_epochs, iq):
    return cc.traced(signal, mode, n_epochs, iq=iq)


@pytest.mark.parametrize("signal,mode,n_epochs,iq", CASES)
def test_model_reproduces_the_oracle_sums_at_the_tracker_taps(signal, mode, n_epochs, iq):
    """tau = (-spc, 0, +spc): the same indices, carrier and samples as oracle.tracking's epoch, so the two float64 evaluations
    differ by NumPy's summation order alone: <= 1e-12 sum |x_k|."""
    s, x, chans, trace, _ = traced(signal, mode, n_epochs, iq)
    assert len(trace) == n_epochs * len(chans)
    xs = cc.samples_of(x, s)
    spc = s.dllCorrelatorSpacing
    for t in trace:
        prn, st = cc.states_of([t], chans)
        z = cc.model(xs, s, mode, prn[0], st[0], [-spc, 0.0, spc])
        want = t["sums"].reshape(3, 3, 2)[: z.shape[0]]  # [comp][E, P, L][I, Q]
        tol = 1e-12 * cc.abs_sum(xs, st[0])
        np.testing.assert_allclose(z.real, want[..., 0], rtol=0, atol=tol)
        np.testing.assert_allclose(z.imag, want[..., 1], rtol=0, atol=tol)
        assert np.all(t["sums"][6 * z.shape[0]:] == 0)


@pytest.mark.parametrize("signal,mode,n_epochs,iq", CASES)
def test_track_states_equal_the_traced_states(signal, mode, n_epochs, iq):
    """Element for element, exactly: pos, blk, rem, codeFreq, remCarr, carrFreq of every epoch of every channel."""
    s, x, chans, trace, res = traced(signal, mode, n_epochs, iq)
    prn, st = bds_amd.track_states(res, chans, s)
    want_prn, want = cc.states_of(sorted(trace, key=lambda t: (t["ch"], t["k"])), chans)
    np.testing.assert_array_equal(prn, want_prn)
    np.testing.assert_array_equal(st, want)
    prn1, st1 = bds_amd.track_states(res, chans, s, epochs=[0, n_epochs - 1])
    keep = [i for i, t in enumerate(sorted(trace, key=lambda t: (t["ch"], t["k"]))) if t["k"] in (1, n_epochs)]
    np.testing.assert_array_equal(st1, want[keep])
    np.testing.assert_array_equal(prn1, want_prn[keep])


def test_track_states_refuses_an_epoch_that_was_not_completed():
    s, x, chans, trace, res = traced("B2A", "B2A", 4, False)
    with pytest.raises(ValueError, match="not completed"):
        bds_amd.track_states(res, chans, s, epochs=[4])
    short = [otrk.tracking(otrk.RawFile(x[: 3 * 25000 + 14000]), chans, s, mode="B2A")[0][0]]
    with pytest.raises(ValueError, match="not completed"):
        bds_amd.track_states(short, chans[:1], s, epochs=[3])


def _clean_record(s, sat, n):
    x = synth.make_if(s, [sat], n, clean=True)
    return np.rint(x * (100.0 / np.abs(x).max())).astype(np.int8)


SHAPE_MARGIN = 0.15  # loose by design: tells a tau in half-chips from chips, and a missing wrap; it does not measure rounding


@functools.lru_cache(maxsize=None)
def shape_case(signal):
    """A noise-free one-satellite record, a few epochs of closed-loop oracle tracking, the last epoch's state."""
    from types import SimpleNamespace

    if signal == "B2A":
        n_ep, mode = 4, "B2A"
        s = bds_amd.init_settings_b2a(samplingFreq=25e6, IF=6.5e6, msToProcess=n_ep, numberOfChannels=1, CNoInterval=20)
        # (the channel starts at the sample after the code's start, as preRun would put it: a delay just below a whole sample keeps
        # the replica within 0.02 chip of the signal -- at 2.44 samples per chip, 3001.2 would leave it a third of a chip off,
        # which a 2-Hz DLL does not pull in within four epochs; nor does it follow the code Doppler, which B2a's channel.codeFreq
        # does not carry: 355 Hz drifts 0.003 chip per epoch, 2210 Hz would drift 0.02)
        sat = synth.Sat(19, 355.0, 3001.95, 0.4, 47.0)
    else:
        n_ep, mode = 3, "NB"
        s = bds_amd.init_settings_b1c(samplingFreq=12.5e6, IF=3.5e6, msToProcess=n_ep * 10, numberOfChannels=1, pilotTRKflag=1,
                                      CNoInterval=10, FEBW=10e6)
        sat = synth.Sat(12, -410.0, 99000.8, 2.0, 45.0)
    spc = int(np.floor(s.samplingFreq / (s.codeFreqBasis / s.codeLength) + 0.5))
    x = _clean_record(s, sat, (n_ep + 3) * spc)
    cf = s.IF + round(sat.doppler / 25) * 25
    code_freq = (s.codeFreqBasis - (cf - s.IF) / s.carrFreqBasis * s.codeFreqBasis) if signal == "B1C" else s.codeFreqBasis
    chans = [SimpleNamespace(PRN=sat.prn, acquiredFreq=float(cf), codePhase=float(int(np.ceil(sat.delay)) + 1), codeFreq=float(code_freq), status="T")]
    res, _ = otrk.tracking(otrk.RawFile(x), chans, s, mode=mode)
    prn, st = bds_amd.track_states(res, chans, s, epochs=[n_ep - 1])
    return s, mode, cc.samples_of(x, s), prn[0], st[0]


def test_shape_b2a_triangle():
    s, mode, xs, prn, st = shape_case("B2A")
    taps = np.array([0, -1, -0.75, -0.5, -0.25, 0.25, 0.5, 0.75, 1, -2, 2, -8, 8, -16, 16], dtype=np.float64)
    z = cc.model(xs, s, mode, prn, st, taps)[0]
    r = np.abs(z) / np.abs(z[0])
    want = np.where(np.abs(taps) <= 1, 1 - np.abs(taps), 0.0)
    print("B2a |R(tau)|/|R(0)|:", dict(zip(taps.tolist(), np.round(r, 3).tolist())))
    assert np.all(np.abs(r - want) <= SHAPE_MARGIN), (r, want)


def test_shape_b1c_boc11_side_peaks():
    s, mode, xs, prn, st = shape_case("B1C")
    taps = np.array([0, -0.5, 0.5], dtype=np.float64)
    z = cc.model(xs, s, mode, prn, st, taps)[0]
    r = (z / z[0]).real
    print("B1C data Re R(tau)/R(0):", dict(zip(taps.tolist(), np.round(r, 3).tolist())))
    assert np.all(np.abs(r[1:] + 0.5) <= SHAPE_MARGIN), r


@pytest.mark.parametrize("variant", cc.VARIANTS)
def test_wrong_rules_are_told_apart(variant):
    """Each deliberate change moves some I or Q of the GPU test's items by more than the GPU tolerance, 1e-6 |P|."""
    mode = {"six_ceil": "WB", "no_sc": "NB"}.get(variant, "B2A")  # (sc = 1 for B2a; BOC(6,1) in wide-band mode only)
    s, x, chans, trace, _ = traced("B2A" if mode == "B2A" else "B1C", mode, 4 if mode == "B2A" else 3, False)
    xs = cc.samples_of(x, s)
    taps = cc.gpu_taps(s.dllCorrelatorSpacing)
    if mode != "B2A":
        taps = taps[[4, 5, 6, 7, 8]]  # (a 125 000-sample block per tap and component: a few taps are enough)
    worst = 0.0
    for t in [t for t in trace if t["ch"] == 0 and t["k"] in (1, 2)]:
        prn, st = cc.states_of([t], chans)
        good = cc.model(xs, s, mode, prn[0], st[0], taps)
        bad = cc.model(xs, s, mode, prn[0], st[0], taps, variant=variant)
        p = abs(good[0, list(taps).index(0.0)])
        worst = max(worst, cc.worst_rel_error(bad[None], good[None], [p]))
    print(f"{variant}: moves some I or Q by {worst:.3e} |P|")
    assert worst > cc.GPU_RTOL, (variant, worst)


def test_entries_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "bds_mi355x.h")).read()
    for entry in ("bds_corr_function", "bds_corr_function_mem"):
        assert re.search(r"BDS_API\s+int\s+%s\s*\(" % entry, src) and entry in native.EXPORTS
    assert re.search(r"BDS_CORR_DEV_API\s+int\s+bds_corr_function_dev\s*\(", src) and native.CORR_DEVICE_EXPORTS == ["bds_corr_function_dev"]
    lib = native.lib()
    for entry in ("bds_corr_function", "bds_corr_function_mem", "bds_corr_function_dev"):
        assert hasattr(lib, entry), entry
    assert hasattr(native.Context, "corr_function") and callable(bds_amd.corr_function) and callable(bds_amd.track_states)
    for text in ("tracking.m:260-316", "WB_tracking.m:289-324", "periodic", "beyond the reference"):
        assert text.lower() in src.lower(), text
