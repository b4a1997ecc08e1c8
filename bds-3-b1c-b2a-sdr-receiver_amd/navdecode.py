"""Navigation decoding over trackResults -- what follows frame synchronisation in the reference:

    B1C  B1C/include/BCNAV1decoding.m:93-189  BCH(21,6) / BCH(51,8) of sub-frame 1 in either polarity, the 36 x 48
         de-interleaver, CRC-24Q of sub-frames 2 and 3, B1C/include/ephemeris.m
    B2a  B2a/include/BCNAV2decoding.m:99-159  five-chip vote per symbol, polarity by the preamble, CRC-24Q,
         B2a/include/ephemeris.m

Every candidate of every channel is decoded in one launch on the GPU (``bds_nav_decode``); the merge into one ephemeris per
channel is host C++.  No CPU fallback.  As in the reference there is NO LDPC decoding: the information halves are taken as
received and stand or fall with their CRC.

One rule is the library's own: a CRC-valid frame whose PRN field is outside 1..63 -- at which the reference's ``ephemeris``
returns early and leaves ``TOW`` empty -- is not entered: it changes nothing and does not set ``firstSubFrame``.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

from . import native
from .acquisition import get_context

SAT_TYPE = ["", "GEO", "IGSO", "MEO"]
# the fields of the two eph_structure_init.m files (bds_eph holds their union)
_B1C_ONLY = {"SOH", "HOW", "IODC", "IODE", "T_GDB2ap", "ISC_B1Cd", "T_GDB1Cp", "PageID1", "PageID3", "SISMAI", "TOW"}
_B2A_ONLY = {"SOW", "IODC_MSB2", "IODC_LSB8"}


def _eph_namespace(d, b1c):
    """eph as the reference's struct: a field the reference leaves [] is None, SatType is '' / 'GEO' / 'IGSO' / 'MEO'."""
    skip = _B2A_ONLY if b1c else _B1C_ONLY
    ns = SimpleNamespace()
    for f in native.EPH_FIELDS:
        if f not in skip:
            setattr(ns, f, None if math.isnan(d[f]) else d[f])
    ns.SatType = SAT_TYPE[d["SatType"]]
    if b1c:
        ns.flag = 1 if d["flag"] else None
    else:
        ns.idValid = d["idValid"].copy()
    return ns


def _prompts(track_results, settings):
    b1c = str(settings.signal).upper() == "B1C"
    chans = [r for r in track_results if int(getattr(r, "PRN", 0) or 0) != 0]  # (an idle channel: PRN 0 or None)
    if not chans:
        return b1c, chans, None, None
    if b1c:
        field = "Pilot_I_P" if int(settings.pilotTRKflag) == 2 else "Pilot_Q_P"  # BCNAV1decoding.m:66-73
        sync = np.stack([np.asarray(getattr(r, field), dtype=np.float64) for r in chans])
        data = np.stack([np.asarray(r.I_P, dtype=np.float64) for r in chans])  # :104
    else:
        sync = np.stack([np.asarray(r.I_P, dtype=np.float64) for r in chans])  # BCNAV2decoding.m:83
        data = None
    return b1c, chans, sync, data


def nav_decode(track_results, settings, device: int = 0, cap: int = 8):
    """One result per tracked channel (PRN != 0) of ``track_results``: a namespace with ``eph`` (a namespace of the signal's
    eph_structure_init fields, None where the reference leaves []), ``firstSubFrame`` and ``TOW`` (inf where nothing
    decoded), ``frames`` (the first ``cap`` candidates: index, status, polarity, bch1_max, bch2_max, bits) and ``n_frames``."""
    b1c, chans, sync, data = _prompts(track_results, settings)
    if not chans:
        return []
    res = get_context(device).nav_decode(settings, [int(r.PRN) for r in chans], sync, data, cap=cap)
    return [SimpleNamespace(eph=_eph_namespace(r["eph"], b1c), firstSubFrame=r["firstSubFrame"], TOW=r["TOW"],
                            frames=[SimpleNamespace(**f) for f in r["frames"]], n_frames=r["n_frames"]) for r in res]


def BCNAV1decoding(trackResults, channelNr, settings, device: int = 0):
    """[eph, firstSubFrame, TOW] = BCNAV1decoding(trackResults, channelNr, settings); channelNr is 1-based."""
    r = nav_decode([trackResults[int(channelNr) - 1]], settings, device=device, cap=0)
    if not r:
        raise ValueError(f"BCNAV1decoding: channel {channelNr} has PRN 0")
    return r[0].eph, r[0].firstSubFrame, r[0].TOW


def BCNAV2decoding(I_P_InputBits, device: int = 0):
    """[eph, firstSubFrame, TOW] = BCNAV2decoding(I_P_InputBits)."""
    from .settings import init_settings_b2a

    tr = [SimpleNamespace(PRN=1, I_P=np.asarray(I_P_InputBits, dtype=np.float64).reshape(-1))]
    r = nav_decode(tr, init_settings_b2a(), device=device, cap=0)
    return r[0].eph, r[0].firstSubFrame, r[0].TOW
