"""The correlation function along a tracked channel (bds_corr_function*, csrc/bds_corrfn.hip): a float64 NumPy model written from
the index rule of include/bds_mi355x.h, the case builders and the assertion, shared by tests/test_corrfn_cases.py (no GPU),
tests/test_corrfn_gpu.py and tests/test_corrfn_mex.py.

The model evaluates every sample (no run identity): the replica index of tap tau is ceil() of the MATLAB colon vector
(rem + tau)*sc : step*sc : (((blk-1)*step + rem) + tau)*sc (oracle.matlab.m_colon), read from the periodic extension of the code
(oracle.codes), the carrier the reference's exp(-+j trigarg)."""
import functools

import numpy as np

from oracle import codes
from oracle import tracking as otrk
from oracle.matlab import m_colon

from helpers import track_case

# deliberate changes of the index rule a correct kernel must NOT match (test_corrfn_cases.py shows each differs from the model)
VARIANTS = ("clamp", "no_sc", "floor", "six_ceil", "neg_tau")

GPU_RTOL = 1e-6  # of |P|: the project's open-loop tolerance (tests/test_track_gpu.py)


def samples_of(x, settings):
    """The record's samples as float64 / complex128 (int8 or int16 values; fileType 2: interleaved I/Q pairs)."""
    x = np.asarray(x)
    if int(settings.fileType) == 2:
        return x[0::2].astype(np.float64) + 1j * x[1::2].astype(np.float64)
    return x.astype(np.float64)


@functools.lru_cache(maxsize=None)
def _codes(signal, mode, prn, pilot):
    import bds_amd

    s = bds_amd.init_settings_b2a() if signal == "B2A" else bds_amd.init_settings_b1c()
    if signal == "B2A":
        out = [codes.generate_b2a_data_code(prn, s)]
        if pilot:
            out.append(codes.generate_b2a_pilot_code(prn, s))
    else:
        out = [codes.generate_data_boc11(s, prn)]
        if pilot:
            out.append(codes.generate_pilot_boc11(s, prn))
            if mode == "WB":
                out.append(codes.generate_pilot_boc61(s, prn))
    return tuple(np.asarray(c, dtype=np.float64) for c in out)


def pilot_of(settings, mode):
    return int(settings.pilotTRKflag) == (2 if mode == "WB" else 1)


def model(x, settings, mode, prn, state6, taps, variant=None):
    """complex128 [n_comp, n_taps]: I + jQ of one item.  x: samples_of(record).  variant: one of VARIANTS, a deliberately wrong rule."""
    pos, blk, rem, code_freq, rem_carr, carr_freq = (float(v) for v in state6)
    pos, blk = int(pos), int(blk)
    fs = float(settings.samplingFreq)
    b2a = mode == "B2A"
    sc = 1.0 if b2a else 2.0
    step = code_freq / fs
    raw = x[pos:pos + blk]
    assert len(raw) == blk
    trig = ((carr_freq * 2.0 * np.pi) * (np.arange(blk, dtype=np.float64) / fs)) + rem_carr
    if b2a:  # exp(+j th): q = real, i = imag (tracking.m:309-314)
        mixed = np.exp(1j * trig) * raw
        i_bb, q_bb = mixed.imag, mixed.real
    else:  # exp(-j th): i = real, q = imag (NB_tracking.m:320-325)
        mixed = np.exp(-1j * trig) * raw
        i_bb, q_bb = mixed.real, mixed.imag
    cs = _codes("B2A" if b2a else "B1C", mode, int(prn), pilot_of(settings, mode))
    out = np.zeros((len(cs), len(taps)), dtype=np.complex128)

    def look(c, u):
        n = len(c)
        if variant == "clamp":  # the reference's padded table [c(L) c(1..L) c(1)], index clamped at its ends
            padded = np.concatenate([[c[-1]], c, [c[0]]])
            return padded[np.clip(u, 0, n + 1)]
        return c[(u - 1) % n]

    for j, tau in enumerate(taps):
        tau = -float(tau) if variant == "neg_tau" else float(tau)
        last = (blk - 1) * step + rem
        if variant == "no_sc":
            t = m_colon(rem * sc + tau, step * sc, last * sc + tau)
        else:
            t = m_colon((rem + tau) * sc, step * sc, (last + tau) * sc)
        assert len(t) == blk
        rnd = np.floor if variant == "floor" else np.ceil
        u = rnd(t).astype(np.int64)
        for comp, c in enumerate(cs):
            if comp == 2:
                u6 = 6 * rnd(t).astype(np.int64) if variant == "six_ceil" else rnd(t * 6).astype(np.int64)
                r = look(c, u6)
            else:
                r = look(c, u)
            out[comp, j] = np.sum(r * i_bb) + 1j * np.sum(r * q_bb)
    return out


def abs_sum(x, state6):
    """sum |x_k| over the item's block: the scale of the summation-order difference between two float64 evaluations."""
    pos, blk = int(state6[0]), int(state6[1])
    return float(np.sum(np.abs(x[pos:pos + blk])))


def traced(signal, mode, n_epochs, iq=False, **kw):
    """(settings, record, channels, trace, results) of the oracle's closed-loop run on helpers.track_case."""
    s, x, chans = track_case(signal, mode, n_epochs, iq=iq, **kw)
    trace = []
    res, _ = otrk.tracking(otrk.RawFile(x), chans, s, mode=mode, trace=trace)
    return s, x, chans, trace, res


def states_of(rows, chans):
    prn = np.array([chans[t["ch"]].PRN for t in rows], dtype=np.int32)
    st = np.array([[t["pos"], t["blk"], t["rem"], t["codeFreq"], t["remCarr"], t["carrFreq"]] for t in rows], dtype=np.float64)
    return prn, st


def gpu_taps(spc):
    """The tap set of the kernel-against-model test: far taps, the integer / half-integer ones, -+spacing, and 33 uniform over -+1.6."""
    return np.array([-16, -8, -1.5, -1, -0.5, -spc, 0, spc, 0.5, 1, 1.5, 8, 16] + list(np.linspace(-1.6, 1.6, 33)), dtype=np.float64)


def worst_rel_error(got, want, p_mag):
    """max over items of max |got - want| (I and Q separately) / |P| of the item."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    p_mag = np.asarray(p_mag, dtype=np.float64)
    assert np.all(p_mag > 0)
    d = got - want
    err = np.maximum(np.abs(d.real), np.abs(d.imag)).reshape(got.shape[0], -1).max(axis=1)
    return float(np.max(err / p_mag))


def assert_close(got, want, p_mag, what=""):
    w = worst_rel_error(got, want, p_mag)
    print(f"corrfn {what}: worst |error| / |P| = {w:.3e}")
    assert w <= GPU_RTOL, (what, w)
    return w
