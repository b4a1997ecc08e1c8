"""notch_tones -- excision of narrow-band (CW) interference from an IF record on the device (bds_notch* of
include/bds_mi355x.h): per block of `block` samples each tone's complex amplitude is estimated and the tone subtracted, on the
record's own bytes, in integers only.  A notched record is an ordinary record; acquisition, tracking, TrackSession, probe_data
and blank_pulses take it as it is.  The record may be a file, a host array or a torch tensor that exists only in device memory;
there is no CPU fallback.  notch_detect takes the tone list from probe_data's PSD, notch_refine corrects the frequencies from
the block estimates of an estimate-only call: detect, notch_tones(estimate_only=True), refine, notch_tones."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from . import native
from .acquisition import get_context


def notch_step(f: float, fs: float) -> int:
    """The uint32 phase step per sample of a tone at f Hz: floor(f / fs 2^32 + 0.5) mod 2^32 (a negative frequency of an I/Q
    record is the two's complement)."""
    return int(math.floor(float(f) / float(fs) * 4294967296.0 + 0.5)) % (1 << 32)


@dataclass
class NotchReport:
    """n_samples, n_blocks: what the call owned; n_saturated: samples clipped to the element's range; sum_sq_in / sum_sq_out: the
    exact sums of x^2 (I^2 + Q^2) before and after (modulo 2^64; sum_sq_out 0 for an estimate-only call); est: complex128
    (n_blocks, n_tones), each tone's amplitude per block in LSB (of a real record half the tone's amplitude: the projection on
    exp(+j phi)); steps: the uint32 phase steps applied; tones: their frequencies in Hz; block: samples per block."""
    n_samples: int
    n_blocks: int
    n_saturated: int
    sum_sq_in: int
    sum_sq_out: int
    est: np.ndarray
    steps: list
    tones: list
    block: int

    @property
    def removed_db(self) -> float:
        """10 log10(sum_sq_in / sum_sq_out): the power the call took out of the record."""
        if not self.sum_sq_out or not self.sum_sq_in:
            return float("nan") if not self.sum_sq_in else float("inf")
        return 10.0 * math.log10(self.sum_sq_in / self.sum_sq_out)


def _block_log2(block) -> int:
    b = int(block)
    if b <= 0 or b & (b - 1):
        raise ValueError(f"block = {block!r}: a power of two from 2^{native.NOTCH_MIN_LOG2} to 2^{native.NOTCH_MAX_LOG2}")
    return b.bit_length() - 1


def notch_tones(source, settings, tones, block=1024, out=None, estimate_only=False, first_sample=0, device=0, n_samples=None,
                piece_samples=0):
    """(record, NotchReport) = notch_tones(source, settings, tones, ...).

    tones: frequencies in Hz on probe_data's axis -- for a real record 0 .. fs / 2, the IF included; for an I/Q record signed
    baseband frequencies.  source: a path (out: the path to write), a host array (out: None for a new array, "inplace", or an
    array of the same bytes) or a torch tensor on the GPU, read and written where it lies (out: None for a new tensor, "inplace",
    or a tensor of the same size); a tensor comes back for a tensor.  estimate_only: nothing is written, the record returned is
    None and the report carries the block estimates.  first_sample: the absolute index of the source's first sample (a multiple
    of block) for a caller working in pieces.  n_samples / piece_samples: files only."""
    fs = float(settings.samplingFreq)
    tones = [float(f) for f in np.atleast_1d(np.asarray(tones, dtype=np.float64))]
    steps = [notch_step(f, fs) for f in tones]
    beta = _block_log2(block)
    apply = not estimate_only
    dst = native.conditioner_out(source, out, "notching a file writes another file: give out=path") if apply else None
    res, r = get_context(device).notch(settings, source, steps, beta, out=dst, first_sample=first_sample, apply=apply,
                       n_samples=-1 if n_samples is None else int(n_samples), piece_samples=piece_samples)
    est = (r["est"][..., 0].astype(np.float64) + 1j * r["est"][..., 1].astype(np.float64)) / float(1 << native.NOTCH_AMP_FRAC)
    return res, NotchReport(n_samples=r["n_samples"], n_blocks=r["n_blocks"], n_saturated=r["n_saturated"], sum_sq_in=r["sum_sq_in"],
                            sum_sq_out=r["sum_sq_out"], est=est, steps=steps, tones=tones, block=1 << beta)


def _running_median(x, span, wrap):
    """Median of x over `span` samples around each one (span odd); the ends see the axis go round (wrap) or mirrored."""
    h = int(span) // 2
    padded = np.pad(x, h, mode="wrap" if wrap else "reflect")
    return np.median(np.lib.stride_tricks.sliding_window_view(padded, 2 * h + 1), axis=1)


def notch_detect(probe_result, settings, ratio_db=8.0, max_tones=8, span=257):
    """The narrow-band lines of probe_data's PSD, in Hz on its axis (an I/Q record's upper half mapped to negative frequencies),
    strongest first, at most max_tones.  The floor is the running median of the PSD over `span` bins; runs of bins more than
    ratio_db above it are merged into one tone at their power-weighted centroid.  Host only.  (The PSD's bins are 3 kHz apart at
    probe_data's parameters and fluctuate by 1 / sqrt(n_segments): with fewer than four segments noise alone crosses 8 dB.)"""
    psd = np.asarray(probe_result.psd, dtype=np.float64)
    freq = np.asarray(probe_result.freq, dtype=np.float64)
    iq = int(settings.fileType) != 1
    if iq:  # -fs / 2 .. fs / 2, so that a line at DC is one run
        h = psd.size // 2
        fs = float(settings.samplingFreq)
        psd, freq = np.concatenate([psd[h:], psd[:h]]), np.concatenate([freq[h:] - fs, freq[:h]])
    else:  # the one-sided density's bins at 0 and fs / 2 are not doubled, and no tone is admitted there
        psd, freq = psd[1:-1], freq[1:-1]
    span = min(int(span), 2 * ((psd.size - 1) // 2) - 1) | 1
    floor = _running_median(psd, span, iq)
    above = psd > floor * 10.0 ** (float(ratio_db) / 10.0)
    edges = np.flatnonzero(np.diff(np.concatenate([[False], above, [False]]).astype(np.int8)))
    found = []
    for a, b in zip(edges[0::2], edges[1::2]):
        w = psd[a:b]
        found.append((float(w.sum()), float((w * freq[a:b]).sum() / w.sum())))
    found.sort(key=lambda t: -t[0])
    return [f for _, f in found[:int(max_tones)]]


def notch_refine(report, settings):
    """The tones' frequencies corrected from the block estimates of a call at report.steps: per tone
    df = angle(sum_b a[b] conj(a[b - 1])) fs / (2 pi B) over the full blocks, added to the frequency the step stands for.
    Unambiguous for |df| < fs / (2 B).  Host only; returns the list of frequencies in Hz."""
    fs = float(settings.samplingFreq)
    B = int(report.block)
    full = int(report.n_samples) // B
    a = np.asarray(report.est)[:full]
    iq = int(settings.fileType) != 1
    out = []
    for k, st in enumerate(report.steps):
        f = st / 4294967296.0 * fs
        if iq and st >= 1 << 31:
            f -= fs
        if full >= 2:
            f += float(np.angle(np.sum(a[1:, k] * np.conj(a[:-1, k])))) * fs / (2.0 * np.pi * B)
        out.append(f)
    return out
