"""``[trackResults, channel] = tracking(fid, channel, settings)`` -- host mirror of
BDS-3_B2a/tracking.m:1, BDS-3_B1C/NB_tracking.m:1, BDS-3_B1C/WB_tracking.m:1 and of
``channel = preRun(acqResults, settings)`` (include/preRun.m:1).

``fid`` may be a file path, an open binary file object (its ``.name`` is used: the
reference seeks absolutely from 'bof', B2a/tracking.m:151-153, so the handle position
is irrelevant), an int8 array holding the raw file bytes (uint8 for the packed
records of ``settings.fileType = 3``; an int16 array of samples -- I, Q pairs for
``fileType = 2`` -- when ``settings.dataType`` is ``'int16'``), or those bytes as a device array (a torch tensor
on the GPU: the record is read where it lies, with the same results).  The result is a list of
per-channel structs with exactly the field set the reference variant creates
(SURVEY.md Appendix D).
"""
from __future__ import annotations

import contextlib
import os
from types import SimpleNamespace

import numpy as np

from . import native
from .acquisition import get_context, packed_bytes


class TrackResults(SimpleNamespace):
    """One element of the trackResults struct array."""


def pre_run(acq_results, settings):
    """channel = preRun(acqResults, settings)  (B1C/include/preRun.m, B2a/include/preRun.m)."""
    ch = native.pre_run(settings, acq_results.carrFreq, acq_results.codePhase, acq_results.peakMetric)
    return [SimpleNamespace(PRN=int(c.PRN), acquiredFreq=float(c.acquiredFreq), codePhase=float(c.codePhase),
                            codeFreq=float(c.codeFreq), status=chr(c.status)) for c in ch]


def _mode(settings, mode):
    if mode is None:
        if str(settings.signal).upper() == "B2A":
            return "B2A"
        return "WB" if int(settings.pilotTRKflag) == 2 else "NB"  # B1C/postProcessing.m:137-143
    return mode


def _round_half_away(x):
    return int(np.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def field_set(settings, mode):
    """(n_epochs, n_cno, per-epoch fields, C/N0 fields) of the reference template
    (B2a/tracking.m:48-93, NB_tracking.m:53-102, WB_tracking.m:53-109)."""
    if mode == "B2A":
        n = int(settings.msToProcess)
        pilot = int(settings.pilotTRKflag) == 1
    else:
        n = _round_half_away(settings.msToProcess / 1000 / settings.intTime)
        pilot = int(settings.pilotTRKflag) == (2 if mode == "WB" else 1)
    m = n // int(settings.CNoInterval)
    ep = ["absoluteSample", "codeFreq", "carrFreq", "I_P", "I_E", "I_L", "Q_E", "Q_P", "Q_L"]
    if pilot:
        ep += ["Pilot_I_P", "Pilot_Q_P"]
        if mode == "WB":
            ep += ["Pilot_I_E", "Pilot_I_L", "Pilot_Q_E", "Pilot_Q_L"]
    ep += ["dllDiscr", "dllDiscrFilt", "pllDiscr", "pllDiscrFilt", "remCodePhase", "remCarrPhase"]
    cn = ["DataCNo", "DataPLD"] + (["PilotCNo", "PilotPLD", "SigCNo"] if pilot else [])
    return n, m, ep, cn, pilot


@contextlib.contextmanager
def _resident_limit(ctx, resident_limit):
    """The context's resident limit set to `resident_limit` bytes for one call (None: left as it is)."""
    if resident_limit is None:
        yield
        return
    before = ctx.track_resident_limit()
    ctx.track_set_resident_limit(resident_limit)
    try:
        yield
    finally:
        ctx.track_set_resident_limit(before)


def _device_record(a, settings, field):
    """A device array as the record's raw bytes, with the dtype rule of the host arrays: uint8 for the packed bytes of
    settings.fileType 3, int16 samples for settings.dataType 'int16', int8 otherwise (checked before any native call)."""
    name = native.device_dtype_name(a)
    w16 = native.record_is_int16(settings, name, field)
    want = "int16" if w16 else "uint8" if int(settings.fileType) == 3 else "int8"
    if name != want:
        raise ValueError(f"{field} must be a {want} device array when settings.fileType is {int(settings.fileType)}"
                         + (" (packed bytes: two 2+2-bit I/Q samples per byte)" if want == "uint8" else "") + f", not {name}")
    return a


def tracking(fid, channel, settings, mode=None, device: int = 0, resident_limit=None):
    """resident_limit: bytes of the IF record that may be resident in HBM during this call -- a larger window is streamed
    through in pieces, bit-identical results (bds_track_set_resident_limit; 0 = no limit).  None leaves the context's
    setting alone: by default a window is held whole when it can be allocated and streamed when it cannot."""
    mode = _mode(settings, mode)
    s = settings.copy() if hasattr(settings, "copy") else settings
    if mode in ("NB", "WB") and str(settings.signal).upper() != "B1C":
        raise ValueError("NB/WB tracking are B1C variants")
    n, m, ep, cn, pilot = field_set(settings, mode)
    if isinstance(fid, (str, bytes, os.PathLike)):
        source = fid
    elif native.is_device_array(fid):
        source = _device_record(fid, settings, "fid")
    elif hasattr(fid, "name") and not isinstance(fid, np.ndarray):
        source = fid.name
    elif int(settings.fileType) == 3:  # packed bytes: never through a conversion to int8 values
        a = np.asarray(fid)
        source = packed_bytes(a.view(np.uint8) if a.dtype == np.int8 else a, field="fid")
    else:  # (int8 bytes, or int16 samples with settings.dataType 'int16': the dtype is checked against the setting before any copy)
        source = _host_values(fid, settings, "fid")
    ctx = get_context(device)
    # the native side derives the variant from settings.signal / pilotTRKflag exactly as
    # postProcessing.m does; an explicit NB request on a pilotTRKflag==2 struct is honoured
    # by passing the flag the variant tests for
    if mode == "NB" and int(s.pilotTRKflag) == 2:
        s = settings.copy(pilotTRKflag=0)
    if mode == "WB" and int(s.pilotTRKflag) != 2:  # WB_tracking.m:78 only tests == 2
        s = settings.copy(pilotTRKflag=0)
    with _resident_limit(ctx, resident_limit):
        arr = ctx.track(s, source, channel, n, m, ep + cn)
    sig_name = "B2a_CNo" if mode == "B2A" else "B1C_CNo"
    out = []
    for c in range(len(channel)):
        r = TrackResults()
        r.status = chr(int(arr["status"][c])) if arr["status"][c] else "-"
        for f in ep:
            setattr(r, f, arr[f][c].copy())
        for f in cn:
            setattr(r, sig_name if f == "SigCNo" else f, arr[f][c].copy())
        r.PRN = int(channel[c].PRN) if int(channel[c].PRN) != 0 else None  # lazily added field, tracking.m:144
        r.completed = int(arr["completed"][c])
        out.append(r)
    return out, channel


def _results(arr, channel_prns, n_ch, ep, cn, mode):
    sig_name = "B2a_CNo" if mode == "B2A" else "B1C_CNo"
    out = []
    for c in range(n_ch):
        r = TrackResults()
        r.status = chr(int(arr["status"][c])) if arr["status"][c] else "-"
        for f in ep:
            setattr(r, f, arr[f][c].copy())
        for f in cn:
            setattr(r, sig_name if f == "SigCNo" else f, arr[f][c].copy())
        r.PRN = int(channel_prns[c]) if int(channel_prns[c]) != 0 else None
        r.completed = int(arr["completed"][c])
        out.append(r)
    return out


def acquire_track(long_signal, path, settings, device: int = 0, resident_limit=None):
    """The acquisition -> preRun -> tracking section of postProcessing.m (B2a/postProcessing.m:100-123,
    B1C/postProcessing.m:105-143) as ONE native call: bds_acquire_track runs the search, allocates the channels with a
    device kernel (bds_pre_run_device) and tracks the record at `path` with the variant the settings select, without
    returning to the host language in between.  Returns (acqResults, channel, trackResults).
    `path` may also be the record's raw bytes, in host memory or as a device array, and long_signal a device array (the record's
    bytes as settings.fileType lays them out): the same three steps then run as three native calls -- the search, bds_pre_run_device,
    bds_track_mem / bds_track_dev -- with the same results.
    resident_limit: as in tracking()."""
    mode = _mode(settings, None)
    n, m, ep, cn, pilot = field_set(settings, mode)
    if native.is_device_array(long_signal) or not isinstance(path, (str, bytes, os.PathLike)):
        from .acquisition import acquisition

        ctx = get_context(device)
        acq = acquisition(long_signal, settings, device=device, verbose=False)
        ch = ctx.pre_run_device(settings, acq.carrFreq, acq.codePhase, acq.peakMetric)
        channel = [SimpleNamespace(PRN=int(c.PRN), acquiredFreq=float(c.acquiredFreq), codePhase=float(c.codePhase),
                                   codeFreq=float(c.codeFreq), status=chr(c.status)) for c in ch]
        results, _ = tracking(path, channel, settings, device=device, resident_limit=resident_limit)
        return acq, channel, results
    x = np.asarray(long_signal)
    is_complex = np.iscomplexobj(x)
    if int(settings.fileType) == 3:  # packed bytes, in the block as in the file
        x, is_complex = packed_bytes(x), 2
    elif is_complex:  # fileType 2: interleaved int8 (dataType 'int16': int16) pairs, as acquisition() hands them over
        pairs = np.empty(2 * x.size, dtype=np.int16 if native.data_type_code(settings.dataType) == 1 else np.int8)
        pairs[0::2], pairs[1::2] = x.real.astype(pairs.dtype), x.imag.astype(pairs.dtype)
        x = pairs
    ctx = get_context(device)
    with _resident_limit(ctx, resident_limit):
        (carr, cph, pm, det), ch, arr = ctx.acquire_track(settings, x if is_complex == 2 else _host_values(x, settings, "longSignal"), is_complex, path, n, m, ep + cn)
    acq = SimpleNamespace(carrFreq=carr, codePhase=cph, peakMetric=pm)
    channel = [SimpleNamespace(PRN=int(c.PRN), acquiredFreq=float(c.acquiredFreq), codePhase=float(c.codePhase),
                               codeFreq=float(c.codeFreq), status=chr(c.status)) for c in ch]
    return acq, channel, _results(arr, [c.PRN for c in channel], len(channel), ep, cn, mode)


def _host_values(x, settings, field):
    """A host array of samples (or of a record's raw bytes) as the int8 row the native calls take, or, with settings.dataType
    'int16', the int16 row; the array's dtype is checked against the setting before any copy (native.record_is_int16)."""
    if native.record_is_int16(settings, np.asarray(x).dtype.name, field):
        return native._i16(x, field)
    return np.ascontiguousarray(x, dtype=np.int8)


class TrackSession:
    """A tracking run whose loop state survives the call (bds_track_open* .. bds_track_close): advance in pieces of any size, or
    on samples fed by the caller.  The concatenation of the arrays of successive ``advance`` calls equals, bit for bit, what ONE
    ``tracking()`` call over the same epochs returns (settings.msToProcess is not read: a session has no preset end, and every
    channel stops at its own short read).

    source: a file path, an open binary file (its ``.name``), or the raw file bytes (int8; uint8 for settings.fileType = 3; int16
    samples for settings.dataType = 'int16'), in
    host memory or as a device array (a torch tensor on the GPU; it must stay unmodified until close()).  ``feed`` takes either kind.
    origin=N (a multiple of 32) instead opens a FEED session: pass source=None; the record is what ``feed`` appends, sample N
    of the record first.  resident_limit: bytes of the record resident in HBM (None: the context's limit, else 256 MiB).
    One session may be open per context; tracking() on that context raises until it is closed."""

    def __init__(self, source, channel, settings, *, origin=None, resident_limit=None, ctx=None, mode=None, device: int = 0):
        self._sess = None
        mode = _mode(settings, mode)
        if mode in ("NB", "WB") and str(settings.signal).upper() != "B1C":
            raise ValueError("NB/WB tracking are B1C variants")
        s = settings
        if mode == "NB" and int(s.pilotTRKflag) == 2:
            s = settings.copy(pilotTRKflag=0)
        if mode == "WB" and int(s.pilotTRKflag) != 2:
            s = settings.copy(pilotTRKflag=0)
        self.mode, self.settings, self.channel = mode, s, list(channel)
        _, _, self._ep, self._cn, _ = field_set(settings, mode)
        self._M = int(settings.CNoInterval)
        if origin is not None:
            if source is not None:
                raise ValueError("a feed session (origin=) has no source: the record is what feed() appends")
            native.check_feed_origin(origin)
        elif source is None:
            raise ValueError("source is required (or origin= for a feed session)")
        self._ctx = ctx if ctx is not None else get_context(device)
        with _resident_limit(self._ctx, resident_limit):  # (read at the open)
            if origin is not None:
                self._sess = self._ctx.track_open_feed(s, origin, self.channel)
            elif isinstance(source, (str, bytes, os.PathLike)):
                self._sess = self._ctx.track_open(s, source, self.channel)
            elif native.is_device_array(source):
                self._sess = self._ctx.track_open(s, _device_record(source, settings, "source"), self.channel)
            elif hasattr(source, "name") and not isinstance(source, np.ndarray):
                self._sess = self._ctx.track_open(s, source.name, self.channel)
            elif int(settings.fileType) == 3:
                a = np.asarray(source)
                self._sess = self._ctx.track_open(s, packed_bytes(a.view(np.uint8) if a.dtype == np.int8 else a, field="source"), self.channel)
            else:
                self._sess = self._ctx.track_open(s, _host_values(source, settings, "source"), self.channel)

    def _open(self):
        if self._sess is None:
            raise native.BdsError(-1, "the tracking session is closed")
        return self._sess

    def feed(self, data, last=False) -> int:
        """Append bytes of the settings' fileType to the record; returns how many were taken (fewer than offered when the
        resident span is full: advance, then feed the rest).  last=True marks the end of the record."""
        sess = self._open()
        if native.is_device_array(data):  # (bds_track_feed_dev; the same argument errors, raised in there before any native call)
            return self._ctx.track_feed(sess, _device_record(data, self.settings, "data"), last)
        native.check_feed_bytes(sess, data)  # (argument errors raise before any native call)
        return self._ctx.track_feed(sess, data, last)

    def advance(self, n):
        """Run the next k <= n epochs of every live channel; returns a TrackResults list with the fields of tracking(), arrays
        cut to the k epochs of this call (C/N0 arrays to the n_cno_done intervals that completed in it); r.completed is the
        number of epochs the channel wrote in this call, self.last_k the k of this call."""
        sess = self._open()
        n = int(n)
        n_cno = (n + self._M - 1) // self._M + 1 if self._M > 1 else 0
        k, arr = self._ctx.track_advance(sess, n, n_cno, self._ep + self._cn)
        self.last_k = k
        out = _results({f: (v[:, :k] if f in self._ep else v) for f, v in arr.items()}, [c.PRN for c in self.channel],
                       len(self.channel), self._ep, self._cn, self.mode)
        sig_name = "B2a_CNo" if self.mode == "B2A" else "B1C_CNo"
        for c, r in enumerate(out):
            r.n_cno_done = int(arr["n_cno_done"][c])
            for f in self._cn:
                f = sig_name if f == "SigCNo" else f
                setattr(r, f, getattr(r, f)[:r.n_cno_done].copy())
        return out

    def info(self) -> dict:
        sess = self._open()
        return self._ctx.track_session_info(sess)

    def close(self) -> None:
        if self._sess is not None:
            self._ctx.track_close(self._sess)
            self._sess = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def NB_tracking(fid, channel, settings, **kw):
    """B1C/NB_tracking.m:1."""
    return tracking(fid, channel, settings, mode="NB", **kw)


def WB_tracking(fid, channel, settings, **kw):
    """B1C/WB_tracking.m:1."""
    return tracking(fid, channel, settings, mode="WB", **kw)
