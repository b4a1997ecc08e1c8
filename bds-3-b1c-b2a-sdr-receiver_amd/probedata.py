"""probe_data -- the numbers behind the reference's probeData figure (include/probeData.m of either receiver): the 257-bin
histogram, the Welch PSD of pwelch(data, 32768, 2048, 32768, fs) and the time-domain excerpt, computed on the device from the
record's own bytes (bds_probe_data* of include/bds_mi355x.h).  The record may be a file, a host array or a torch tensor that
exists only in device memory; there is no CPU fallback."""
from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np

from . import native
from .acquisition import get_context

NFFT, OVERLAP = 32768, 2048


@dataclass
class ProbeResult:
    """hist_i / hist_q: int64[257] over `bins` = -128 .. 128 (hist_q None for a real record); psd: density per Hz over `freq`
    (one-sided 16385 bins of a real record, two-sided 32768 bins 0 .. fs in natural order of an I/Q record); excerpt: the first
    n_time samples (float64, complex128 for I/Q); min / max / mean / rms: floats for a real record, (I, Q) pairs for I/Q, from
    the exact integer sums kept in `sums`."""
    hist_i: np.ndarray
    hist_q: np.ndarray | None
    bins: np.ndarray
    psd: np.ndarray
    freq: np.ndarray
    n_segments: int
    n_samples: int
    excerpt: np.ndarray
    min: object
    max: object
    mean: object
    rms: object
    sums: dict

    def psd_shifted(self):
        """(frequency, psd) of an I/Q record reordered to -fs/2 .. fs/2 as probeData.m:132-134 plots it."""
        h = self.freq.size // 2
        return np.concatenate([-self.freq[h - 1::-1][:h], self.freq[:h]]), np.concatenate([self.psd[h:], self.psd[:h]])


def samples_per_code(settings) -> int:
    """probeData.m:66-67 (MATLAB round: half away from zero)."""
    return int(np.floor(settings.samplingFreq / (settings.codeFreqBasis / settings.codeLength) + 0.5))


def excerpt_length(settings) -> int:
    """Samples of the time-domain plot: B2a/include/probeData.m:96 round(spc / 500) for a real record, :106 round(spc / 2) for I/Q;
    B1C/include/probeData.m:96,106 round(spc / 2) for both."""
    spc = samples_per_code(settings)
    real_b2a = int(settings.fileType) == 1 and str(getattr(settings, "signal", "")).upper() != "B1C"
    return int(np.floor(spc / (500 if real_b2a else 2) + 0.5))


def probe_data(*args, n_samples=None, n_time=None, device=0) -> ProbeResult:
    """probe_data(settings) | probe_data(fileNameStr, settings) | probe_data(array_or_tensor, settings).

    n_samples (files only): None = the window the signal's probeData.m reads (5 code periods for B2a, 10 for B1C), an int, or
    "all" = to the end of the file.  An array or tensor is probed whole (slice it to probe a part).  A torch tensor on the GPU
    is read where it lies (bds_probe_data_dev).  n_time: samples of the excerpt (default: the reference's plot length, capped
    at the window)."""
    if len(args) == 1:
        settings = args[0]
        source = settings.fileName
    elif len(args) == 2:
        source, settings = args
    else:
        raise TypeError("Incorect number of arguments")  # (probeData.m:53)
    ctx = get_context(device)
    is_path = isinstance(source, (str, bytes, os.PathLike))
    if is_path:
        ns = 0 if n_samples is None else -1 if n_samples == "all" else int(n_samples)
        if ns < 0 and n_samples != "all":
            raise ValueError(f"n_samples = {n_samples!r}: None, a count or \"all\"")
    elif n_samples is not None:
        raise ValueError("n_samples applies to files; an array or tensor is probed whole")
    else:
        ns = 0
    if n_time is None:
        n_time = excerpt_length(settings)
        if is_path and ns > 0:
            n_time = min(n_time, ns)
        elif not is_path:
            if native.is_device_array(source):
                n_bytes = native.device_record(settings, source, ctx.device)[1]
            else:
                n_bytes = native.record_bytes(settings, source)[0].size
            w16 = native.data_type_code(getattr(settings, "dataType", "schar")) == 1
            bits = {1: 8, 2: 16, 3: 4}[int(settings.fileType)] * (2 if w16 else 1)
            n_time = min(n_time, n_bytes * 8 // bits)
    r = ctx.probe_data(settings, source, n_time, ns)
    cplx = r["hist_q"] is not None
    n = r["n_samples"]
    fs = float(settings.samplingFreq)
    freq = np.arange(r["psd"].size) * (fs / NFFT)
    comps = "iq" if cplx else "i"
    mean = [r[f"sum_{c}"] / n for c in comps]
    rms = [float(np.sqrt(r[f"sumsq_{c}"] / n)) for c in comps]
    mn, mx = [r[f"min_{c}"] for c in comps], [r[f"max_{c}"] for c in comps]
    one = (lambda v: tuple(v)) if cplx else (lambda v: v[0])
    return ProbeResult(hist_i=r["hist_i"], hist_q=r["hist_q"], bins=np.arange(-128, 129), psd=r["psd"], freq=freq, n_segments=r["n_segments"],
                       n_samples=n, excerpt=r["excerpt_re"] + 1j * r["excerpt_im"] if cplx else r["excerpt_re"], min=one(mn), max=one(mx),
                       mean=one(mean), rms=one(rms), sums={k: v for k, v in r.items() if k[:3] in ("sum", "min", "max")})
