"""The pulse blanker's model and cases (shared by tests/test_blank_cases.py and tests/test_blank_gpu.py): the rule of
include/bds_mi355x.h "pulse blanking" restated in NumPy, once straight from the definition and once with a difference array,
the four record formats, and the builders of the records the device is held to."""
from types import SimpleNamespace

import numpy as np

import bds_amd
from bds_amd import native, synth

T = native.BLANK_TILE

# name -> (fileType, dataType, NumPy dtype of the elements, components per sample)
FORMATS = {"s8": (1, "schar", np.int8, 1), "s8c": (2, "schar", np.int8, 2), "s16": (1, "int16", np.dtype("<i2"), 1), "s16c": (2, "int16", np.dtype("<i2"), 2)}


def settings_of(fmt, **kw):
    ft, dt, _, _ = FORMATS[fmt]
    return bds_amd.init_settings_b2a(fileType=ft, dataType=dt, **kw)


def power(rec, fmt):
    """p[n] of a record given as its element array (int8 / int16, pairs interleaved): exact, as uint64."""
    v = np.asarray(rec).astype(np.int64)
    c = FORMATS[fmt][3]
    return (v.reshape(-1, c) ** 2).sum(axis=1).astype(np.uint64)


def blanked_brute(flag, pre, post):
    """Straight from the definition: n is blanked when a flagged m has m - pre <= n <= m + post."""
    n = flag.size
    out = np.zeros(n, dtype=bool)
    for k in range(n):
        out[k] = flag[max(0, k - post):min(n, k + pre + 1)].any()
    return out


def blanked_fast(flag, pre, post):
    """The same with a difference array: +1 at m - pre, -1 behind m + post, blanked where the running sum is positive."""
    n = flag.size
    d = np.zeros(n + 1, dtype=np.int64)
    m = np.flatnonzero(flag)
    np.add.at(d, np.maximum(m - pre, 0), 1)
    np.add.at(d, np.minimum(m + post + 1, n), -1)
    return np.cumsum(d[:n]) > 0


def model(rec, fmt, threshold_sq, pre, post, lead=0, tail=0, duty_samples=0, blanked=blanked_fast):
    """(the blanked record, report) of one buffer: the first `lead` and last `tail` samples are read for flags only."""
    rec = np.asarray(rec)
    c = FORMATS[fmt][3]
    flag = power(rec, fmt) > np.uint64(threshold_sq)
    n = flag.size
    state = blanked(flag, pre, post)            # the rule's verdict on every sample of the buffer
    own = np.zeros(n, dtype=bool)
    own[lead:n - tail] = True
    b = state & own
    out = rec.copy().reshape(-1, c)
    out[b] = 0
    before = np.concatenate([[False], state[:-1]])
    rep = {"n_samples": int(own.sum()), "n_flagged": int((flag & own).sum()), "n_blanked": int(b.sum()),
           "n_runs": int((b & ~before).sum()), "duty": None}
    if duty_samples:
        w = b[lead:n - tail]
        nb = -(-w.size // duty_samples)
        rep["duty"] = np.add.reduceat(w.astype(np.int32), np.arange(0, max(w.size, 1), duty_samples))[:nb].astype(np.int32) if w.size else np.zeros(0, np.int32)
    return out.reshape(rec.shape), rep


def pieces(rec, fmt, threshold_sq, pre, post, piece, lead_ctx, tail_ctx):
    """The record worked on `piece` samples at a time, every piece with lead_ctx / tail_ctx samples of raw context (as far as
    the record goes): (the joined record, summed n_flagged, n_blanked, n_runs)."""
    rec = np.asarray(rec)
    c = FORMATS[fmt][3]
    n = rec.size // c
    out, tot = [], np.zeros(3, dtype=np.int64)
    for a in range(0, n, piece):
        b = min(n, a + piece)
        l0, l1 = max(0, a - lead_ctx), min(n, b + tail_ctx)
        o, r = model(rec[l0 * c:l1 * c], fmt, threshold_sq, pre, post, lead=a - l0, tail=l1 - b)
        out.append(o[(a - l0) * c:(b - l0) * c])
        tot += [r["n_flagged"], r["n_blanked"], r["n_runs"]]
    return np.concatenate(out), tuple(int(v) for v in tot)


def quiet(fmt, n, seed=0, amp=3):
    """A record of n samples of small noise (|v| <= amp): nothing near any threshold the cases use."""
    _, _, dt, c = FORMATS[fmt]
    return np.random.default_rng(seed).integers(-amp, amp + 1, n * c).astype(dt)


def with_hits(fmt, n, hits, value=100, seed=0):
    """quiet() with the samples `hits` raised to `value` (first component; the second keeps its noise)."""
    rec = quiet(fmt, n, seed)
    c = FORMATS[fmt][3]
    for h in hits:
        rec[h * c] = value
    return rec


def small_cases():
    """(name, fmt, record, threshold_sq, pre, post) on records short enough for the brute-force model."""
    out = []
    for fmt in FORMATS:
        n = 300
        out += [("none", fmt, quiet(fmt, n), 50 * 50, 3, 5), ("all", fmt, np.full_like(quiet(fmt, n), 100), 0, 0, 0), ("nonzero", fmt, quiet(fmt, n), 0, 0, 0),
                ("ends", fmt, with_hits(fmt, n, [0, n - 1]), 2500, 4, 7), ("zero_window", fmt, with_hits(fmt, n, [5, 6, 100]), 2500, 0, 0),
                ("pre_only", fmt, with_hits(fmt, n, [50, 200]), 2500, 9, 0), ("post_only", fmt, with_hits(fmt, n, [50, 200]), 2500, 0, 9),
                ("one_run", fmt, with_hits(fmt, n, [100, 100 + 3 + 5 + 1]), 2500, 3, 5), ("two_runs", fmt, with_hits(fmt, n, [100, 100 + 3 + 5 + 2]), 2500, 3, 5),
                ("wide", fmt, with_hits(fmt, n, [150]), 2500, 400, 400)]
    return out


def dme_scenario():
    """The jammed B2a record of the issue: settings, the clean record, the jammed one, threshold, pre, post (see
    tests/test_oracle_golden.py::test_acquisition_recovers_injected_satellite for the clean scene, here at 44 dB-Hz)."""
    s = bds_amd.init_settings_b2a(samplingFreq=25e6, IF=6.5e6, acqSatelliteList=[9, 14], acqSearchBand=2000, fineNoncoh=5)
    spc = int(np.floor(s.samplingFreq / (s.codeFreqBasis / s.codeLength) + 0.5))
    clean = synth.make_if(s, [synth.Sat(9, -1230.0, 12345.6, 2.0, 44.0)], 8 * spc, seed=2)
    p = synth.dme_pulses(s, 8 * spc, pairs_per_s=20000, peak=400, f_offset=1e6, seed=7)
    jammed = np.clip(np.rint(clean.astype(np.float64) + p), -127, 127).astype(np.int8)
    return SimpleNamespace(settings=s, spc=spc, clean=clean, jammed=jammed, threshold=100, pre=25, post=25)
