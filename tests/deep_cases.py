"""Weak-signal acquisition (bds_acq_deep; include/bds_mi355x.h "weak-signal acquisition"): the rules restated in NumPy float64 on
the oracle's coarse rows, the scenes and the tolerance functions shared by tests/test_deep_cases.py (no GPU),
tests/test_deep_gpu.py and tests/test_deep_plans_gpu.py.  Bins and lags are 0-based in here; ``fbin`` and ``codePhase`` of a result are 1-based as in the reference.
"""
import contextlib
import functools
import os
import re
from types import SimpleNamespace

import numpy as np

import bds_amd
from bds_amd import synth
from oracle import acquisition as oacq
from oracle import codes
from oracle.matlab import m_round, m_var


def is_b1c(s):
    return str(s.signal).upper() == "B1C"


def sizes(s):
    """(spc, X, N, s2c)"""
    spc = codes.samples_per_code(s)
    if is_b1c(s):
        x_len, n = int(m_round(spc / 10 * s.acqCohT)), int(m_round(spc / 10 * (10 + s.acqCohT)))
    else:
        x_len, n = spc, 2 * spc
    return spc, x_len, n, int(np.ceil(s.samplingFreq / s.codeFreqBasis)) * 2


def as_samples(x, s):
    """The record as the float64 / complex128 row the oracle takes (int8 I/Q pairs for fileType 2)."""
    x = np.asarray(x)
    if int(getattr(s, "fileType", 1)) == 2 and not np.iscomplexobj(x):
        return x[0::2].astype(np.float64) + 1j * x[1::2].astype(np.float64)
    return x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)


def shifts(s, n_blocks, compensate=True, sign=1):
    """sh[k][b] = rint(k spc (frq[b] - IF) / carrFreqBasis); sign = -1 is the deliberately wrong model of the tests."""
    spc = codes.samples_per_code(s)
    frq = oacq.freq_bins(s)
    if not compensate:
        return np.zeros((n_blocks, len(frq)), dtype=np.int64)
    k = np.arange(n_blocks, dtype=np.float64)[:, None] * spc
    return (sign * np.rint(k * (frq[None, :] - s.IF) / s.carrFreqBasis)).astype(np.int64)


def block_rows(x, s, prn, k, bins=None):
    """m_k[b] for the bins asked for: the reference's results(b, :) on block k, the carrier phase from the block's first sample."""
    spc, _, n, _ = sizes(s)
    blk = x[k * spc: k * spc + n]
    assert blk.size == n
    rows = oacq.b1c_coarse_rows if is_b1c(s) else oacq.b2a_coarse_rows
    return dict(rows(blk, s, prn, bins))


def surface(x, s, prn, n_blocks, compensate=True, bins=None, power=True, sign=1):
    """(S[b][l] over `bins` (default all), sum_k (max m_k)^2, the bins): S = sum_k m_k[b][(l - sh) mod N]^2 -- power=False adds
    amplitudes instead (the wrong model)."""
    _, _, n, _ = sizes(s)
    frq = oacq.freq_bins(s)
    bins = list(range(len(frq))) if bins is None else list(bins)
    sh = shifts(s, n_blocks, compensate, sign)
    out = np.zeros((len(bins), n))
    tol_sum = 0.0
    for k in range(n_blocks):
        rows = block_rows(x, s, prn, k, bins)
        tol_sum += max(float(r.max()) for r in rows.values()) ** 2
        for i, b in enumerate(bins):
            out[i] += np.roll(rows[b] ** 2 if power else rows[b], int(sh[k, b]))
    return out, tol_sum, bins


def decide(surf, s, bins=None, images=True):
    """Peak cell and statistics of a surface: fbin (index into its rows), l0, S_peak, S_second (B2a), mu, S_sec, deepMetric.
    images=False is the wrong population that forgets the peak's images one code period away."""
    spc, _, n, s2c = sizes(s)
    fbin = int(np.argmax(surf.max(axis=1)))
    l0 = int(np.argmax(surf.max(axis=0)))
    peak = float(surf[:, l0].max())
    lag = np.arange(n)
    d = (lag - l0) % (spc if images else n)
    pop = np.minimum(d, (spc if images else n) - d) >= s2c
    vals = surf[:, pop]
    mu, sec = float(np.mean(vals)), float(vals.max())
    second = None
    if not is_b1c(s):  # B2a/acquisition.m:224-249
        cp = l0 + 1
        e1, e2, e3, e4 = cp - s2c, cp + s2c, cp - spc + s2c, cp + spc - s2c
        left = np.arange(max(1, e3), e1 + 1) if e1 >= 1 else np.arange(0)
        right = np.arange(e2, min(e4, n) + 1) if e2 < n else np.arange(0)
        second = float(np.max(surf[fbin][np.concatenate([left, right]).astype(np.int64) - 1]))
    return SimpleNamespace(fbin=fbin, l0=l0, peak=peak, second=second, mu=mu, sec=sec, deepMetric=(peak - mu) / (sec - mu))


def sig_power2(x, s, n_blocks):
    """sum_k sigPower_k^2, sigPower_k the reference's line 150 on block k."""
    spc, x_len, _, _ = sizes(s)
    return sum(np.sqrt(m_var(x[k * spc: k * spc + x_len]) * x_len) ** 2 for k in range(n_blocks))


def fine_grid(s):
    n = int(m_round(s.acqStep / 25))
    return -s.acqStep + 25.0 * np.arange(2 * n + 1) if is_b1c(s) else -s.acqStep / 2 + 25.0 * np.arange(n + 1)


def fine_weights(s):
    if not is_b1c(s):
        return 1.0, 1.0
    return (11 / 40, 29 / 40) if int(s.pilotACQflag) == 1 else (1.0, 0.0)


def fine(x, s, prn, n_blocks, l0, fbin, compensate=True, weights=None):
    """F over the fine grid around frq[fbin]; a sample index outside the record counts as zero."""
    spc = codes.samples_per_code(s)
    wd, wp = fine_weights(s) if weights is None else weights
    if is_b1c(s):
        cd, cp = codes.make_data_table(s, prn), codes.make_pilot_table(s, prn)
    else:
        cd, cp = codes.make_b2a_data_table(prn, s), codes.make_b2a_pilot_table(prn, s)
    sh = shifts(s, n_blocks, compensate)
    frq = oacq.freq_bins(s)[fbin] + fine_grid(s)
    n = np.arange(spc, dtype=np.float64)
    out = np.zeros(len(frq))
    for k in range(n_blocks):
        a = l0 + k * spc - int(sh[k, fbin])
        idx = a + np.arange(spc)
        ok = (idx >= 0) & (idx < x.size)
        seg = np.where(ok, x[np.clip(idx, 0, x.size - 1)], 0)
        for j, f in enumerate(frq):
            w = seg * np.exp(2j * np.pi * np.fmod(f * n / s.samplingFreq, 1.0))
            out[j] += (wd * abs(np.sum(w * cd)) + wp * abs(np.sum(w * cp))) ** 2
    return out


def model(x, s, n_blocks, threshold, compensate=True, prns=None, keep=False):
    """{prn: result} of the whole rule: fbin / codePhase (1-based), peakMetric, deepMetric, detected, carrFreq, F, tol (the surface
    tolerance of that PRN: 2e-5 sum_k (max m_k)^2), margin = S_peak - S_sec, and the surface itself with keep=True."""
    x = as_samples(x, s)
    _, _, n, _ = sizes(s)
    assert x.size >= n + n_blocks * codes.samples_per_code(s)
    out = {}
    for prn in (prns or [int(p) for p in s.acqSatelliteList]):
        surf, tol_sum, _ = surface(x, s, prn, n_blocks, compensate)
        d = decide(surf, s)
        r = SimpleNamespace(fbin=d.fbin + 1, codePhase=d.l0 + 1, deepMetric=d.deepMetric, detected=d.deepMetric > threshold,
                            peak=d.peak, mu=d.mu, sec=d.sec, tol=2e-5 * tol_sum, margin=d.peak - d.sec, carrFreq=0.0, F=None,
                            peakMetric=np.sqrt(d.peak / (sig_power2(x, s, n_blocks) if is_b1c(s) else d.second)))
        if r.detected:
            r.F = fine(x, s, prn, n_blocks, d.l0, d.fbin, compensate)
            r.carrFreq = float(oacq.freq_bins(s)[d.fbin] + fine_grid(s)[int(np.argmax(r.F))]) or 1.0
        if keep:
            r.surface = surf
        out[prn] = r
    return out


def deep_metric_bound(r):
    """|deepMetric error| when every surface value errs by at most r.tol: the peak and S_sec move by tol each, mu by at most tol."""
    return r.deepMetric * 2 * r.tol * (1 / (r.peak - r.mu) + 1 / (r.sec - r.mu))


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def b2a_settings(prns, band=2000, step=400, **kw):
    return bds_amd.init_settings_b2a(samplingFreq=25e6, IF=6.5e6, acqSatelliteList=list(prns), acqSearchBand=band, acqStep=step, **kw)


def b1c_settings(prns, band=200, **kw):
    return bds_amd.init_settings_b1c(samplingFreq=12.5e6, IF=3.2e6, acqSatelliteList=list(prns), acqSearchBand=band, **kw)


@functools.lru_cache(maxsize=None)
def mixed_b2a(iq=False):
    """PRN 9 at 46 dB-Hz, PRN 14 at 36 dB-Hz (+830 Hz, delay 20321.3), PRN 21 absent; K = 16."""
    s = b2a_settings([9, 14, 21], fileType=2 if iq else 1)
    sats = [synth.Sat(9, -1230.0, 12345.6, 2.0, 46.0), synth.Sat(14, 830.0, 20321.3, 0.7, 36.0)]
    x = synth.make_if(s, sats, 20 * 25000, seed=2, iq_sign=-1 if iq else 0)
    x.setflags(write=False)
    return s, x, 16


@functools.lru_cache(maxsize=None)
def mixed_b1c():
    """PRN 12 at 35 dB-Hz (-110 Hz, delay 99000.8), PRN 7 absent; K = 8."""
    s = b1c_settings([12, 7])
    x = synth.make_if(s, [synth.Sat(12, -110.0, 99000.8, 2.0, 35.0)], 11 * 125000, seed=2)
    x.setflags(write=False)
    return s, x, 8


@functools.lru_cache(maxsize=None)
def high_doppler_b2a():
    """38 dB-Hz at +9170 Hz: the code drifts 0.195 samples per period, 11.7 over the K = 60 blocks."""
    s = b2a_settings([14], band=10000)
    x = synth.make_if(s, [synth.Sat(14, 9170.0, 20321.3, 0.7, 38.0)], 63 * 25000, seed=2)
    x.setflags(write=False)
    return s, x, 60


@functools.lru_cache(maxsize=None)
def small_b2a():
    """The surface-value scene: 2 PRNs, 11 bins, K = 3."""
    s = b2a_settings([9, 14])
    sats = [synth.Sat(9, -1230.0, 12345.6, 2.0, 47.0), synth.Sat(14, 830.0, 20321.3, 0.7, 45.0)]
    x = synth.make_if(s, sats, 6 * 25000, seed=4)
    x.setflags(write=False)
    return s, x, 3


@functools.lru_cache(maxsize=None)
def small_b1c(pilot=1):
    """1 PRN, 5 bins, K = 2, with the pilot component and without."""
    s = b1c_settings([12], band=100, pilotACQflag=pilot)
    x = synth.make_if(s, [synth.Sat(12, 60.0, 99000.8, 2.0, 45.0)], 5 * 125000, seed=5)
    x.setflags(write=False)
    return s, x, 2


@functools.lru_cache(maxsize=None)
def wrap_b2a():
    """5 bins 5 kHz apart, K = 6: sh reaches +-1; the satellite starts at delay 0.4, so its peak sits at lag 0 or 1 and the shifted
    rows wrap around the ends of the surface."""
    s = b2a_settings([9], band=10000, step=5000)
    x = synth.make_if(s, [synth.Sat(9, 4900.0, 0.4, 1.0, 46.0)], 9 * 25000, seed=6)
    x.setflags(write=False)
    return s, x, 6


# ---- 12 MS/s (B2a: spc 12000, N 24000, s2c 4) and 5 MS/s (B1C: spc 50000, s2c 10): a model costs about a second -----------------
def b2a12_settings(prns, band=2000, step=500, **kw):
    return bds_amd.init_settings_b2a(samplingFreq=12e6, IF=3e6, acqSatelliteList=list(prns), acqSearchBand=band, acqStep=step, **kw)


def b1c5_settings(prns, coh_t, band, **kw):
    return bds_amd.init_settings_b1c(samplingFreq=5e6, IF=1.3e6, acqSatelliteList=list(prns), acqCohT=coh_t, acqSearchBand=band, **kw)


@functools.lru_cache(maxsize=None)
def plans_b2a():
    """The plan-matrix scene (tests/test_deep_plans_gpu.py): 2 PRNs, 9 bins, K = 3, need = N + X - 1 = 35999.  Model: PRN 9 bin 3,
    codePhase 7004, deepMetric 6.54; PRN 14 bin 7, codePhase 8323, deepMetric 5.16; margin / tolerance 37041 and 37871."""
    s = b2a12_settings([9, 14])
    sats = [synth.Sat(9, -1230.0, 7001.6, 2.0, 47.0), synth.Sat(14, 830.0, 20321.3, 0.7, 45.0)]
    x = synth.make_if(s, sats, 6 * 12000, seed=4)
    x.setflags(write=False)
    return s, x, 3


@functools.lru_cache(maxsize=None)
def plans_b1c(pilot=1):
    """B1C with acqCohT = 2 (X 10000, N 60000, need 69999), 1 PRN, 5 bins 250 Hz apart, K = 2, with the pilot component and without.
    Model: bin 3, codePhase 31004; deepMetric 8.56 with the pilot (margin / tolerance 43160), 2.82 without (30755)."""
    s = b1c5_settings([12], 2, 500, pilotACQflag=pilot)
    x = synth.make_if(s, [synth.Sat(12, 60.0, 31001.8, 2.0, 47.0)], 4 * 50000, seed=5)
    x.setflags(write=False)
    return s, x, 2


@functools.lru_cache(maxsize=None)
def drift_b2a():
    """Both ends of a 14 kHz band in 2 kHz steps (15 bins), K = 16: sh spans -2 .. +2 and is non-zero at both detected bins.
    PRN 9 at +14000 Hz (bin 15), PRN 14 at -14000 Hz (bin 1), 44 dB-Hz.  Model: codePhase 7003 / 8323, deepMetric 9.35 / 14.99,
    margin / tolerance 25544 / 40009; without the alignment (compensate = 0) codePhase 7002 / 8325, deepMetric 9.31 / 9.21."""
    s = b2a12_settings([9, 14], band=14000, step=2000)
    sats = [synth.Sat(9, 14000.0, 7001.6, 2.0, 44.0), synth.Sat(14, -14000.0, 20321.3, 0.7, 44.0)]
    x = synth.make_if(s, sats, 19 * 12000, seed=3)
    x.setflags(write=False)
    return s, x, 16


@functools.lru_cache(maxsize=None)
def shift_b2a():
    """The wrap_b2a idea taken to the end, unphysical by design: carrFreqBasis = 6001 Hz makes sh fill the allowed range --
    9 bins 500 Hz apart, K = 4, max |sh| = rint(36000 x 2000 / 6001) = 11998 = spc - 2 -- so every row is added at its own offset
    (l + sh) mod N, over both wraps.  (6000 Hz reaches spc: refused.)  The satellite sits on the centre bin, the one row sh leaves
    alone, so that the scene has a peak: PRN 9 at +60 Hz, 47 dB-Hz; bin 5, codePhase 7004, deepMetric 6.08, margin / tolerance 39819."""
    s = b2a12_settings([9], carrFreqBasis=6001.0)
    x = synth.make_if(b2a12_settings([9]), [synth.Sat(9, 60.0, 7001.6, 1.0, 47.0)], 7 * 12000, seed=6)
    x.setflags(write=False)
    return s, x, 4


EDGES = {"edge_b2a_left": (2.3, 6), "edge_b2a_first": (11998.6, 6), "edge_b2a_image": (0.4, 6), "edge_b2a_right": (11993.2, 7)}


@functools.lru_cache(maxsize=None)
def edge_b2a(name):
    """The peak at an end of the surface, where the B2a second-peak ranges (B2a/acquisition.m:224-249) are clipped: one satellite at
    47 dB-Hz and +700 Hz, 9 bins, K = 4; the record has exactly N + K spc samples (the last block's window ends with it).  Model
    (delay, seed -> codePhase, deepMetric, margin / tolerance), EDGES in order:
      2.3, 6 -> 4, 11.61, 41598 (left range empty);     11998.6, 6 -> 1, 9.79, 41937 (left range empty);
      0.4, 6 -> 12002, 10.07, 36391 (l0 >= spc);        11993.2, 7 -> 23995, 9.37, 40456 (right range clipped at N, l0 >= spc)."""
    delay, seed = EDGES[name]
    s = b2a12_settings([9])
    x = synth.make_if(s, [synth.Sat(9, 700.0, delay, 1.0, 47.0)], 6 * 12000, seed=seed)
    x.setflags(write=False)
    return s, x, 4


def edge_conditions(s, code_phase):
    """Which clipped cases of the second-peak ranges a peak at code_phase (1-based) meets: (left range empty, right range clipped
    at N, l0 >= spc)."""
    spc, _, n, s2c = sizes(s)
    return code_phase - s2c < 1, code_phase + s2c < n < code_phase + spc - s2c, code_phase - 1 >= spc


@functools.lru_cache(maxsize=None)
def coh10_b1c(pilot=0, iq=False):
    """B1C with acqCohT = 10 (X 50000, N 100000), 5 bins 50 Hz apart, K = 2: PRN 12 at +60 Hz, delay 31001.8, 40 dB-Hz -- without the
    pilot on a real record, with it on an I/Q record, without it on an I/Q record (iq_sign = -1).  Model: bin 4, codePhase 31004 in
    all three; deepMetric 6.40 / 45.13 / 16.24, margin / tolerance 40088 / 48680 / 44538."""
    s = b1c5_settings([12], 10, 100, pilotACQflag=pilot, fileType=2 if iq else 1)
    x = synth.make_if(s, [synth.Sat(12, 60.0, 31001.8, 2.0, 45.0)], 4 * 50000 + 100, seed=5, iq_sign=-1 if iq else 0)
    x.setflags(write=False)
    return s, x, 2


@functools.lru_cache(maxsize=None)
def chunks_b2a():
    """201 bins 100 Hz apart, K = 2, one satellite at +8000 Hz (bin 181): on a forced 1280 x 324 plan the inter-pass buffer takes 161
    bins, so the bin loop of every block runs twice and the peak lies in the second chunk.  Model: bin 184 (the 1 ms blocks resolve 1 kHz: the
    bins around 181 are near-equal and the noise picks), codePhase 19003, deepMetric 4.47, margin / tolerance 33126."""
    s = b2a12_settings([9], band=10000, step=100)
    x = synth.make_if(s, [synth.Sat(9, 8000.0, 7001.6, 1.0, 47.0)], 5 * 12000, seed=8)
    x.setflags(write=False)
    return s, x, 2


GPU_SCENES = {"mixed_b2a": mixed_b2a, "mixed_b1c": mixed_b1c, "small_b2a": small_b2a, "small_b1c": small_b1c,
              "small_b1c_nopilot": functools.partial(small_b1c, 0), "wrap_b2a": wrap_b2a,
              "plans_b2a": plans_b2a, "plans_b1c": plans_b1c, "plans_b1c_nopilot": functools.partial(plans_b1c, 0),
              "drift_b2a": drift_b2a, "shift_b2a": shift_b2a, **{name: functools.partial(edge_b2a, name) for name in EDGES},
              "coh10_b1c_nopilot": coh10_b1c, "coh10_b1c_iq": functools.partial(coh10_b1c, 1, True),
              "coh10_b1c_nopilot_iq": functools.partial(coh10_b1c, 0, True), "chunks_b2a": chunks_b2a}
THRESHOLD = 1.5


@functools.lru_cache(maxsize=None)
def scene_model(name, compensate=True):
    """The model of a GPU scene, computed once per session and shared (treat as read-only)."""
    s, x, k = GPU_SCENES[name]()
    return model(x, s, k, THRESHOLD, compensate, keep=True)


# ---- noise floor ----------------------------------------------------------------------------------------------------------------------
def noise_floor(s, ks, seeds):
    """Noise-only deepMetric of the first PRN of s for every K in ks (ascending) and every seed: {K: [values]}; the surfaces of the
    smaller K are the partial sums of the largest."""
    spc, _, n, _ = sizes(s)
    prn = int(s.acqSatelliteList[0])
    out = {k: [] for k in ks}
    for seed in seeds:
        x = synth.make_if(s, [], n + max(ks) * spc, seed=seed).astype(np.float64)
        sh = shifts(s, max(ks))
        surf = np.zeros((len(oacq.freq_bins(s)), n))
        for k in range(max(ks)):
            rows = block_rows(x, s, prn, k)
            for b, r in rows.items():
                surf[b] += np.roll(r ** 2, int(sh[k, b]))
            if k + 1 in out:
                out[k + 1].append(decide(surf, s).deepMetric)
    return out


# ---- the device side against the model (tests/test_deep_gpu.py, tools/deep_errors.py) -------------------------------------------------
def run_scene(name, keep_surface=True, stale=False, **kw):
    """acquisition_deep on a GPU scene with the scenes' threshold.  stale=True: on its record read backwards (no satellite in it)
    and a sampling frequency 1 Hz off -- the same sizes, other values, and another key for the library's cached plan."""
    s, x, k = GPU_SCENES[name]()
    if stale:
        s, x = s.copy(samplingFreq=s.samplingFreq + 1.0), np.ascontiguousarray(x[::-1])
        assert sizes(s) == sizes(GPU_SCENES[name]()[0])
    if int(getattr(s, "fileType", 1)) == 2:  # (a host I/Q record is handed over as complex values)
        x = as_samples(x, s)
    return bds_amd.acquisition_deep(x, s, k, THRESHOLD, keep_surface=keep_surface, **kw)


STALE_PLAN = "64x8000"  # L = 512000: above the need of every scene in here; single-wave columns like the planner's own choices


def _force(ctx, plan):
    os.environ.pop("BDS_ACQ_FORCE_L1L2", None)
    if plan:
        os.environ["BDS_ACQ_FORCE_L1L2"] = plan
    ctx.reload_tuning()


def run_scene_on_stale_surfaces(name, plan=None, **kw):
    """run_scene with keep_surface on the column plan `plan` (BDS_ACQ_FORCE_L1L2 of the test-hooks build; None: the planner's choice)
    into surfaces that hold other values, written through ANOTHER plan.  The library never zeroes a surface (block 0 stores), so a
    value the column pass does not write keeps what the buffer held -- after an earlier test on the same scene, quite possibly the
    right value.  Hence: release everything; the stale run (run_scene) on the planner's plan, or on STALE_PLAN when that is the plan
    under test; then the scene itself, whose other sampling frequency makes deep_configure plan again -- under the forced plan --
    while the surface buffer of the kept stale run, of the same size, stays.  What a pass with a hole in its tiling leaves in the hole
    was put there by a pass with another tiling.  The plan lines of a verbose context (verbose_plans) name both plans."""
    ctx = bds_amd.get_context(0)
    ctx.acq_deep_release()
    try:
        _force(ctx, None if plan else STALE_PLAN)
        run_scene(name, stale=True, **kw)
        _force(ctx, plan)
        return run_scene(name, **kw)
    finally:
        _force(ctx, None)


# The column plans tests/test_deep_plans_gpu.py forces on plans_b2a (need 35999), each within the planner's own limits (5-smooth,
# L1 <= 1280, L2 <= 8192, L2 >= L1 / 4): L1 x L2 -> (T, tiles, columns of the last tile) of k_cols_deep as deep_plan lays it out.
PLANS_B2A = {"8x4500": (16, 282, 4), "256x144": (16, 9, 16), "375x96": (16, 6, 16), "512x135": (16, 9, 7), "768x200": (16, 13, 8),
             "1024x270": (16, 17, 14), "1280x324": (8, 41, 4)}
_PLAN_LINE = re.compile(r"\[bds\] plan: need (\d+) -> L (\d+) = (\d+) \(cols:[^)]*\) x (\d+) \(rows:")


def plans_that_ran(stderr_text):
    """[(need, L1, L2)] of the library's verbose plan lines ([bds] plan: need .. -> L .. = L1 (cols: ..) x L2 (rows: ..))."""
    out = []
    for need, ell, l1, l2 in _PLAN_LINE.findall(stderr_text):
        assert int(ell) == int(l1) * int(l2)
        out.append((int(need), int(l1), int(l2)))
    return out


@contextlib.contextmanager
def verbose_plans(ctx):
    """BDS_VERBOSE for the runs inside: the plan line on stderr says which plan ran -- a forced plan the library does not take falls
    back to the planner's without a word.  On the way out the variables are gone and the deep search is released: deep_configure
    keys its plan on signal, rates, cohT and pilot, not on the tuning, and nothing later may inherit a forced plan."""
    old = os.environ.pop("BDS_VERBOSE", None)
    os.environ["BDS_VERBOSE"] = "1"
    try:
        ctx.reload_tuning()
        yield
    finally:
        os.environ.pop("BDS_VERBOSE", None)
        if old is not None:
            os.environ["BDS_VERBOSE"] = old
        _force(ctx, None)
        ctx.acq_deep_release()


def surface_errors(name, compensate=True, plan=None):
    """Every surface value of a scene (run on stale surfaces, on column plan `plan`) against the model through bds_acq_deep_row:
    {prn: worst |error| / tolerance of that PRN}."""
    s, _, _ = GPU_SCENES[name]()
    _, _, n, _ = sizes(s)
    run_scene_on_stale_surfaces(name, plan, compensate=compensate)
    ctx = bds_amd.get_context(0)
    out = {}
    for prn, r in scene_model(name, compensate).items():
        worst = 0.0
        for b in range(r.surface.shape[0]):
            row = ctx.acq_deep_row(prn, b + 1, n)
            assert row.shape == (n,) and row.dtype == np.float32
            worst = max(worst, float(np.max(np.abs(row.astype(np.float64) - r.surface[b]))) / r.tol)
        out[prn] = worst
    return out
