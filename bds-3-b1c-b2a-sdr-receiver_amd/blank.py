"""blank_pulses -- pulse blanking of an IF record on the device (bds_blank* of include/bds_mi355x.h): every sample within
[m - pre, m + post] of a sample m whose power x^2 (I^2 + Q^2) exceeds threshold^2 is set to 0.  B2a shares its band with DME /
TACAN beacons, whose pulse pairs stand tens of dB above the noise; a blanked record is an ordinary record, and acquisition,
tracking, TrackSession and probe_data take it as it is.  The record may be a file, a host array or a torch tensor that exists
only in device memory; there is no CPU fallback.  blank_threshold takes the threshold from probe_data's histogram."""
from __future__ import annotations

import math
import os
from dataclasses import dataclass

import numpy as np

from . import native
from .acquisition import get_context


@dataclass
class BlankReport:
    """n_samples: the samples the call owned (the buffer's without lead and tail); n_flagged: those above the threshold;
    n_blanked: those set to 0; n_runs: maximal runs of blanked samples (the pulse count); duty: int32 blanked samples per
    duty_samples (None when not asked for); threshold_sq, pre, post: what was applied."""
    n_samples: int
    n_flagged: int
    n_blanked: int
    n_runs: int
    duty: np.ndarray | None
    threshold_sq: int
    pre: int
    post: int

    @property
    def fraction(self) -> float:
        return self.n_blanked / self.n_samples if self.n_samples else 0.0


def _kappa(c: float) -> float:
    """sqrt(E[v^2 | |v| <= c sigma]) / sigma of a Gaussian: the truncated-Gaussian correction."""
    p = math.erf(c / math.sqrt(2.0))
    return math.sqrt(1.0 - 2.0 * c * math.exp(-0.5 * c * c) / (math.sqrt(2.0 * math.pi) * p))


def robust_sigma(hist, bins=None, c: float = 1.5, iterations: int = 100) -> float:
    """A noise sigma from a histogram that pulses have contaminated: 1.4826 x MAD to begin with, then
    sigma <- sqrt(mean of v^2 over |v| <= c sigma) / kappa(c) to its fixed point."""
    h = np.asarray(hist, dtype=np.float64)
    v = np.arange(-128, 129, dtype=np.float64) if bins is None else np.asarray(bins, dtype=np.float64)
    if h.sum() <= 0:
        raise ValueError("an empty histogram")
    total = h.sum()
    med = v[np.searchsorted(np.cumsum(h) / total, 0.5)]
    # the median of |v - med|, a bin taken as the interval of width 1 around its value: linear inside the bin that crosses 1/2
    dev = np.abs(v - med)
    order = np.argsort(dev, kind="stable")
    d_sorted, uniq = np.unique(dev[order], return_index=True)
    mass = np.add.reduceat(h[order], uniq) / total
    cum = np.cumsum(mass)
    j = int(np.searchsorted(cum, 0.5))
    below = cum[j - 1] if j else 0.0
    width = 0.5 if d_sorted[j] == 0 else 1.0  # (|v - med| = 0 covers [0, 1/2), every other value [d - 1/2, d + 1/2))
    mad = max(d_sorted[j] - 0.5, 0.0) + width * (0.5 - below) / mass[j]
    sigma = max(1.4826 * mad, 0.5)
    k = _kappa(c)
    for _ in range(iterations):
        sel = np.abs(v) <= c * sigma
        w = h[sel].sum()
        if w <= 0:
            break
        new = math.sqrt(float((h[sel] * v[sel] ** 2).sum() / w)) / k
        if abs(new - sigma) <= 1e-9 * sigma:
            sigma = new
            break
        sigma = new
    return float(sigma)


def blank_threshold(probe_result, k: float = 5.0, settings=None) -> float:
    """k x the robust noise sigma of a record, from probe_data's exact histogram (for an I/Q record the rms of the two components'
    sigmas, the amplitude |I + jQ| is compared with).  A 16-bit record's values lie outside the 257 bins (the histogram clamps
    them): pass settings to have that refused here, and give blank_pulses a number."""
    if settings is not None and native.data_type_code(getattr(settings, "dataType", "schar")) == 1:
        raise ValueError("blank_threshold: the 257-bin histogram clamps a dataType 'int16' record; pass blank_pulses a number")
    if max(abs(int(np.min(probe_result.min))), abs(int(np.max(probe_result.max)))) > 128:
        raise ValueError("blank_threshold: the record's values leave the 257 bins (a 16-bit record); pass blank_pulses a number")
    si = robust_sigma(probe_result.hist_i, probe_result.bins)
    if probe_result.hist_q is None:
        return k * si
    sq = robust_sigma(probe_result.hist_q, probe_result.bins)
    return k * math.sqrt(0.5 * (si * si + sq * sq))


def blank_pulses(source, settings, threshold=None, pre=None, post=None, out=None, duty_samples=None, lead=0, tail=0, device=0,
                 n_samples=None, piece_samples=0):
    """(record, BlankReport) = blank_pulses(source, settings, ...).

    source: a path (out: the path to write), a host array (out: None for a new array, "inplace", or an array of the same bytes)
    or a torch tensor on the GPU, read and written where it lies (out: None for a new tensor, "inplace", or a tensor of the same
    size); a tensor comes back for a tensor.  threshold: an amplitude, threshold_sq = floor(threshold^2); None: 5 sigma from
    probe_data of the source (blank_threshold; int8 records).  pre / post: samples blanked in front of / behind every hit,
    default round(1e-6 samplingFreq) each.  lead / tail: samples at the ends of the buffer that are context only.
    n_samples / piece_samples: files only (the window behind settings.skipNumberOfBytes; None: to the end of the file)."""
    ctx = get_context(device)
    us = int(math.floor(1e-6 * float(settings.samplingFreq) + 0.5))
    pre = us if pre is None else int(pre)
    post = us if post is None else int(post)
    is_path = isinstance(source, (str, bytes, os.PathLike))
    if threshold is None:
        from .probedata import probe_data

        threshold = blank_threshold(probe_data(source, settings, n_samples="all", n_time=0, device=device) if is_path
                                    else probe_data(source, settings, n_time=0, device=device), settings=settings)
    if not (threshold >= 0):
        raise ValueError(f"threshold = {threshold!r}")
    tsq = min(int(math.floor(float(threshold) ** 2)), 2 ** 32 - 1)
    dst = native.conditioner_out(source, out, "blanking a file writes another file: give out=path")
    res, r = ctx.blank(settings, source, tsq, pre, post, out=dst, lead=lead, tail=tail, duty_samples=duty_samples or 0,
                       n_samples=-1 if n_samples is None else int(n_samples), piece_samples=piece_samples)
    return res, BlankReport(threshold_sq=tsq, pre=pre, post=post, **r)
