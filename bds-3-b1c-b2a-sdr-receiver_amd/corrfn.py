"""The correlation function along a tracked channel: an open-loop replay of tracked epochs at any set of tap offsets
(bds_corr_function*, include/bds_mi355x.h).  The trackers return, per epoch, the Early / Prompt / Late sums at
-+dllCorrelatorSpacing and everything needed to run the epoch again: ``track_states`` turns trackResults into the (prn, state6)
items of the native call, ``corr_function`` evaluates them at the caller's taps.  Beyond the reference: its loops have no
taps but E, P and L (B2a/tracking.m:260-316, B1C/WB_tracking.m:289-324).
"""
from __future__ import annotations

import os

import numpy as np

from . import native
from .acquisition import get_context, packed_bytes
from .tracking import _device_record, _host_values, _mode


def track_states(track_results, channel, settings, epochs=None):
    """(prn, state6) of the chosen epochs of every live channel, channel by channel: prn int32 [n_items], state6 float64
    [n_items, 6] = {sample offset, blksize, remCodePhase, codeFreq, remCarrPhase, carrFreq} -- the NCO state epoch e was
    correlated WITH.  All five are epoch e's own entries: absoluteSample, remCodePhase and remCarrPhase are stored before the
    sample loop, and codeFreq / carrFreq are stored just BEFORE the loop filters replace them (tracking.m:361-363,387-389;
    WB_tracking.m:404-406,428-430), so entry e holds what epoch e ran on -- entry 0 channel.codeFreq / channel.acquiredFreq.
    epochs: 0-based indices (default: every epoch of msToProcess); one that a channel did not complete is refused."""
    fs = float(settings.samplingFreq)
    code_len = int(settings.codeLength)
    prn, st = [], []
    for r, ch in zip(track_results, channel):
        if int(ch.PRN) == 0:
            continue
        n_all = len(r.absoluteSample)
        done = int(getattr(r, "completed", np.count_nonzero(np.isfinite(np.asarray(r.carrFreq, dtype=np.float64)))))
        es = range(n_all) if epochs is None else [int(e) for e in np.atleast_1d(epochs)]
        for e in es:
            if not 0 <= e < done:
                raise ValueError(f"PRN {int(ch.PRN)}: epoch {e} was not completed (the channel finished {done} of {n_all})")
            code_freq, carr_freq = float(r.codeFreq[e]), float(r.carrFreq[e])
            rem = float(r.remCodePhase[e])
            blk = int(np.ceil((code_len - rem) / (code_freq / fs)))  # tracking.m:230-233
            prn.append(int(ch.PRN))
            st.append([float(r.absoluteSample[e]), float(blk), rem, code_freq, float(r.remCarrPhase[e]), carr_freq])
    return np.asarray(prn, dtype=np.int32), np.asarray(st, dtype=np.float64).reshape(-1, 6)


def qmboc_composite(pilot11, pilot61):
    """WB_tracking.m:375-380 on complex sums I + jQ: I = -sqrt(4/33) I61 + sqrt(29/33) Q11, Q = -sqrt(4/33) Q61 - sqrt(29/33) I11."""
    a, b = np.sqrt(4 / 33), np.sqrt(29 / 33)
    p, s = np.asarray(pilot11), np.asarray(pilot61)
    return (-a * s.real + b * p.imag) + 1j * (-a * s.imag - b * p.real)


def corr_function(source, channel, settings, track_results, taps, epochs=None, composite=False, mode=None, device: int = 0):
    """R(tau) of the chosen epochs of every live channel of a tracking run: complex128 [n_items, n_comp, n_taps], I + jQ of the raw
    sums, items in the order of track_states (channel by channel, epochs ascending).  taps: offsets in primary-code chips, the
    unit of dllCorrelatorSpacing (at most 128, |tau| <= 16).  comp 0 is the data component, comp 1 the pilot when the pilot
    correlators are on, comp 2 the pilot BOC(6,1) in wide-band mode.  composite=True (wide-band mode): comp 1 is the QMBOC
    composite of WB_tracking.m:375-380 instead -- what Pilot_I_E .. Pilot_Q_L hold -- formed here from the two pilot components,
    and the result has two components.  source: what tracking() takes -- a path, an open binary file, the raw bytes, or those bytes
    as a device array."""
    mode = _mode(settings, mode)
    s = settings
    if mode in ("NB", "WB") and str(settings.signal).upper() != "B1C":
        raise ValueError("NB/WB tracking are B1C variants")
    if mode == "NB" and int(s.pilotTRKflag) == 2:
        s = settings.copy(pilotTRKflag=0)
    if mode == "WB" and int(s.pilotTRKflag) != 2:
        s = settings.copy(pilotTRKflag=0)
    if composite and not (mode == "WB" and int(s.pilotTRKflag) == 2):
        raise ValueError("composite=True: the QMBOC composite exists in wide-band mode (pilotTRKflag = 2) only")
    if isinstance(source, (str, bytes, os.PathLike)):
        src = source
    elif native.is_device_array(source):
        src = _device_record(source, settings, "source")
    elif hasattr(source, "name") and not isinstance(source, np.ndarray):
        src = source.name
    elif int(settings.fileType) == 3:
        a = np.asarray(source)
        src = packed_bytes(a.view(np.uint8) if a.dtype == np.int8 else a, field="source")
    else:
        src = _host_values(source, settings, "source")
    prn, st = track_states(track_results, channel, settings, epochs)
    z = get_context(device).corr_function(s, src, prn, st, taps)
    if composite:
        z = np.stack([z[:, 0], qmboc_composite(z[:, 1], z[:, 2])], axis=1)
    return z
