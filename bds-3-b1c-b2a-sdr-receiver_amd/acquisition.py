"""``acqResults = acquisition(longSignal, settings)`` -- host mirror of
BDS-3_B2a/acquisition.m:1, BDS-3_B1C/acquisition.m:1 and BDS-3_B1C/GPU_acquisition.m:1.

Same arguments, same result fields (``carrFreq``, ``codePhase``, ``peakMetric``: 1 x
max(acqSatelliteList), zeros where not searched / not detected), same console line
``(19 20 . )``.  The work is done by libbds_mi355x.so; this file only converts types.
"""
from __future__ import annotations

import sys
from types import SimpleNamespace

import numpy as np

from . import native

_ctx = {}


def get_context(device: int = 0) -> native.Context:
    """Process-wide bds_ctx per device (keeps the code-spectrum cache warm across calls)."""
    if device not in _ctx:
        _ctx[device] = native.Context(device)
    return _ctx[device]


def release_context(device: int = 0) -> None:
    """Destroy the process-wide context of a device (its HBM -- IF block, code spectra, the inter-pass buffer of the search --
    goes back to the device); the next call builds a new one."""
    c = _ctx.pop(device, None)
    if c is not None:
        c.close()


class AcqResults(SimpleNamespace):
    """acqResults struct (B2a/acquisition.m:161-165)."""


def packed_bytes(long_signal, field="longSignal"):
    """The uint8 bytes of a packed record (settings.fileType 3: two 2+2-bit I/Q samples per byte, B2a/include/unpack_cplx.m:18-30).
    Sample values -- real or complex -- are refused: the packed format carries bytes, as fread(fid, n, 'uint8=>uint8') returns them."""
    a = np.asarray(long_signal)
    if a.dtype != np.uint8:
        raise ValueError(f"{field} must be a uint8 array of packed bytes when settings.fileType is 3 (two 2+2-bit I/Q samples per "
                         f"byte), not {a.dtype}: unpacked samples go with fileType 1 or 2")
    return np.ascontiguousarray(a).reshape(-1)


def _as_int8(long_signal, settings):
    """The block as the int8 (settings.dataType 'int16': int16) row the native entries take, and is_complex."""
    if int(getattr(settings, "fileType", 1)) == 3:
        native.record_is_int16(settings, np.asarray(long_signal).dtype.name, "longSignal")  # (int16 settings: uint8 bytes disagree)
        return packed_bytes(long_signal), 2
    a = np.asarray(long_signal)
    w16 = native.record_is_int16(settings, a.dtype.name, "longSignal")  # dtype against settings.dataType, before any copy
    if np.iscomplexobj(a):
        # fileType 2: data = I + 1i*Q (B2a/postProcessing.m:92-96)
        inter = np.empty(a.size * 2, dtype=np.float64)
        inter[0::2] = a.real
        inter[1::2] = a.imag
        a, is_complex = inter, True
    else:
        is_complex = False
    if w16:
        if a.dtype != np.int16:
            r = np.rint(a)
            if not np.array_equal(r, a) or r.min() < -32768 or r.max() > 32767:
                raise ValueError("longSignal must hold int16 values (fread(...,'int16'))")
            a = r.astype(np.int16)
        return np.ascontiguousarray(a).reshape(-1), is_complex
    if a.dtype != np.int8:
        r = np.rint(a)
        if not np.array_equal(r, a) or r.min() < -128 or r.max() > 127:
            raise ValueError("longSignal must hold int8 values (fread(...,'schar'), postProcessing.m:89-90)")
        a = r.astype(np.int8)
    return np.ascontiguousarray(a).reshape(-1), is_complex


def _device_block(long_signal, settings):
    """A device array as the block: the record's bytes as settings.fileType lays them out -- 1: real int8 samples, 2: interleaved
    I/Q int8 pairs, 3: packed uint8 bytes -- under the dtype rule of the host arrays (int16 with settings.dataType 'int16')."""
    ft = int(getattr(settings, "fileType", 1))
    a = long_signal
    name = native.device_dtype_name(a)
    w16 = native.record_is_int16(settings, name, "longSignal")
    want = "int16" if w16 else "uint8" if ft == 3 else "int8"
    if name != want:
        raise ValueError(f"longSignal must be a {want} device array when settings.fileType is {ft}, not {name}")
    return a, 2 if ft == 3 else ft == 2


def acquisition(long_signal, settings, device: int = 0, prn_list=None, verbose: bool = True, b2a_npoint=None, b1c_npoint=None) -> AcqResults:
    """Parallel code-phase search acquisition on the GPU.

    long_signal: the samples as the reference hands them over (real, or complex for an I/Q record; uint8 packed bytes for
    settings.fileType 3), or (extension) a device array -- a torch tensor on the GPU holding the record's bytes as
    settings.fileType lays them out -- which is searched where it lies (bds_acq_load_dev), with the same results.

    prn_list (extension): the PRN shard this rank searches; results are zero outside
    the shard so an all-reduce(SUM) over ranks reassembles acqResults.
    b2a_npoint (extension): True / False sets the device context's opt-in N-point search for B2a at 99.375 MS/s
    (Context.acq_set_b2a_npoint; it stays set for later calls), None leaves the context as it is (off unless set).
    b1c_npoint (extension): the same for the opt-in N-point search for B1C at 30.69 MS/s (Context.acq_set_b1c_npoint).
    """
    ctx = get_context(device)
    if b2a_npoint is not None:
        ctx.acq_set_b2a_npoint(b2a_npoint)
    if b1c_npoint is not None:
        ctx.acq_set_b1c_npoint(b1c_npoint)
    samples, is_complex = _device_block(long_signal, settings) if native.is_device_array(long_signal) else _as_int8(long_signal, settings)
    ctx.acq_load(settings, samples, is_complex)
    ctx.acq_prepare(settings)
    carr, cph, pm, det = ctx.acq_run(settings, prn_list)
    if verbose:  # B2a/acquisition.m:167,259,360,366
        sats = [int(p) for p in (np.atleast_1d(settings.acqSatelliteList) if prn_list is None else prn_list)]
        sys.stdout.write("(" + "".join(f"{p:02d} " if det[p - 1] else ". " for p in sats) + ")\n")
    return AcqResults(carrFreq=carr, codePhase=cph, peakMetric=pm)


def acquisition_deep(long_signal, settings, n_blocks, threshold, compensate=True, keep_surface=False, surface_gib=0.0, device: int = 0,
                     verbose: bool = False) -> AcqResults:
    """Weak-signal acquisition (extension; include/bds_mi355x.h "weak-signal acquisition"): the coarse search's squared surfaces of
    n_blocks blocks one code period apart are added -- aligned per Doppler bin by the code drift unless compensate=False -- and a PRN
    is detected when deepMetric, (peak - mean) / (largest other value - mean) of its surface, exceeds `threshold` (> 1; the README
    lists noise-only values).  long_signal: as for acquisition(), int8 real or I/Q, a NumPy array or a torch tensor in HBM, at least
    N + n_blocks * samplesPerCode samples.  Returns the acqResults fields -- carrFreq and codePhase zero where not detected, so the
    result feeds pre_run unchanged -- plus deepMetric and fbin (1-based).  keep_surface=True keeps the surfaces for
    get_context(device).acq_deep_row; acq_deep_fine gives a detected PRN's fine-frequency sums."""
    ctx = get_context(device)
    samples, is_complex = _device_block(long_signal, settings) if native.is_device_array(long_signal) else _as_int8(long_signal, settings)
    carr, cph, pm, dm, fb, det = ctx.acq_deep(settings, samples, is_complex, n_blocks, threshold, compensate, keep_surface, surface_gib)
    if verbose:
        sys.stdout.write("(" + "".join(f"{int(p):02d} " if det[int(p) - 1] else ". " for p in np.atleast_1d(settings.acqSatelliteList)) + ")\n")
    return AcqResults(carrFreq=carr, codePhase=cph, peakMetric=pm, deepMetric=dm, fbin=fb)


def GPU_acquisition(long_signal, settings, **kw) -> AcqResults:
    """B1C/GPU_acquisition.m:1 -- same native entry as acquisition()."""
    return acquisition(long_signal, settings, **kw)
