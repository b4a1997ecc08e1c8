"""Position fix over trackResults -- the reference's last processing step:

    BDS-3_B1C/postNavigation.m, BDS-3_B2a/postNavigation.m  decoding per channel, readiness, measurement grid, the fix chain
    Common/calculatePseudoranges.m                          index search, transmit time, raw pseudoranges
    include/satpos.m, include/check_t.m                     satellite position and clock
    Common/leastSquarePos.m (+ e_r_corr, topocent, togeod, tropo), Common/cart2geo.m

The measurement stage (one lane per measurement epoch and channel: search, transmit time, satpos) runs on the GPU in one launch
(``bds_pvt_measure``); the chain that is sequential over the epochs (local time, elevation mask, least squares, DOP, geodetic
coordinates) is host C++ (``bds_pvt_solve``).  No CPU fallback for the device stage.  UTM coordinates (``utmZone``, ``E``, ``N``,
``U``) are not computed: latitude / longitude / height and ECEF are.

Rules that are the library's own (include/bds_mi355x.h): for B2a the ``T_GDB1Cp`` term of satpos is 0 (the
B2a ephemeris has no such field); a ready channel with an empty ``SatType`` is dropped; ``absoluteSample`` must increase strictly
on every ready channel; two channels with the same PRN are two rows.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from . import native
from .acquisition import get_context
from .navdecode import _eph_namespace, _prompts

RECORD_GATE_MS = {"B1C": 36000, "B2A": 24000}  # BDS-3_B1C/postNavigation.m:49, BDS-3_B2a/postNavigation.m:50

pvt_plan = native.pvt_plan
pvt_solve = native.pvt_solve


def pvt_measure(settings, ready, absolute_sample, code_freq, rem_code_phase, ephs, sub_frame_start, tow, sample_start,
                meas_sample_step, n_meas, device: int = 0):
    """The device stage alone: (transmitTime [n_meas, n_ch], satPos [n_meas, n_ch, 3], satClkCorr [n_meas, n_ch])."""
    return get_context(device).pvt_measure(settings, ready, absolute_sample, code_freq, rem_code_phase, ephs, sub_frame_start, tow,
                                           sample_start, meas_sample_step, n_meas)


def _tracked(r):
    return str(getattr(r, "status", "-") or "-")[:1] != "-" and int(getattr(r, "PRN", 0) or 0) != 0


def post_navigation(track_results, settings, device: int = 0):
    """[navSolutions, eph] = postNavigation(trackResults, settings).

    ``navSolutions`` is a namespace of float64 arrays: PRN, el, az, transmitTime, satClkCorr, rawP, correctedP
    [numberOfChannels, n_meas]; DOP [5, n_meas]; X, Y, Z, dt, localTime, currMeasSample, latitude, longitude, height [n_meas];
    and ``channelStatus``, the BDS_PVT_* flags per channel.  It is None when fewer than 4 channels are ready or no measurement
    epoch fits.  ``eph`` is a dict by PRN of the decoded ephemerides.  Below the record-length gate both are None."""
    sig = str(settings.signal).upper()
    for name in ["msToProcess"] + native.PVT_SETTINGS:
        if not hasattr(settings, name):
            raise AttributeError(f"settings.{name} is missing")
    if settings.msToProcess < RECORD_GATE_MS[sig]:
        return None, None
    rows = list(track_results)
    active = [c for c, r in enumerate(rows) if _tracked(r)]  # :69
    if not active:
        return None, {}
    ctx = get_context(device)
    b1c, chans, sync, data = _prompts([rows[c] for c in active], settings)
    dec = ctx.nav_decode(settings, [int(r.PRN) for r in chans], sync, data, cap=0)  # :78-79
    n_ch = len(rows)
    n = len(np.asarray(rows[active[0]].absoluteSample).reshape(-1))
    series = {f: np.zeros((n_ch, n)) for f in ("absoluteSample", "codeFreq", "remCodePhase")}
    ephs, sfs, tow = [None] * n_ch, np.full(n_ch, np.inf), np.full(n_ch, np.inf)
    eph = {}
    for c, d in zip(active, dec):
        for f, a in series.items():
            v = np.asarray(getattr(rows[c], f), dtype=np.float64).reshape(-1)
            if v.size != n:
                raise ValueError(f"post_navigation: channel {c + 1} has {v.size} values of {f}, channel {active[0] + 1} has {n}")
            a[c] = v
        ephs[c], sfs[c], tow[c] = d["eph"], d["firstSubFrame"], d["TOW"]
        eph[int(rows[c].PRN)] = _eph_namespace(d["eph"], b1c)
    status = "".join("T" if c in active else "-" for c in range(n_ch))
    prns = [int(getattr(r, "PRN", 0) or 0) for r in rows]
    arrays, ready = ctx.post_navigation(settings, status, prns, series["absoluteSample"], series["codeFreq"], series["remCodePhase"],
                                        ephs, sfs, tow)
    if arrays is None:
        return None, eph
    return SimpleNamespace(channelStatus=ready, **arrays), eph


postNavigation = post_navigation
