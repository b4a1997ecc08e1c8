"""Tracking sessions (bds_track_open* .. bds_track_close): the piece lists and records the tests use, and a NumPy model of "which
C/N0 intervals complete in which call" with the carry a session keeps between calls.

The model restates what the library carries, not how: per channel the prompts of the unfinished interval and the raw values of
the last finished one.  An interval that ends in a call is evaluated over the carried prompts followed by the call's, in epoch
order, by the oracle's Calc_CNo_PLD restatement; the two-point smoothing takes its "previous" value across call boundaries."""
import functools
from types import SimpleNamespace

import numpy as np

import bds_amd
from bds_amd import synth
from oracle import tracking as otrk

# piece lists per total number of epochs: the sizes cross every interval boundary of the CNoInterval they are used with
PIECES = {
    60: [[1, 7, 13, 39], [60], [1] * 60],  # B2a, CNoInterval = 10
    12: [[5, 1, 6]],                        # B1C, CNoInterval = 4
}
CNO_INTERVAL = {60: 10, 12: 4}
FEED_CHUNK = 1_000_003  # bytes, a prime
FEED_ADVANCE = 1000


def n_cno_done(pieces, M):
    """Intervals that complete in each call: floor((e0 + k) / M) - floor(e0 / M), e0 = the epochs done before it."""
    out, e0 = [], 0
    for k in pieces:
        out.append((e0 + k) // M - e0 // M)
        e0 += k
    return out


def whole_series_cno(i_p, q_p, pil_i, pil_q, settings, pilot_mode):
    """(CNo [m, 3] smoothed, PLD [m, 2]) of a whole prompt series, as oracle.tracking's epoch loop forms them (tracking.m:411-434)."""
    M = int(settings.CNoInterval)
    m = len(i_p) // M
    cno, pld = np.zeros((m, 3)), np.zeros((m, 2))
    prev = np.zeros(3)
    for q in range(m):
        sl = slice(q * M, (q + 1) * M)
        val, det = otrk.calc_cno_pld(i_p[sl], q_p[sl], pil_i[sl], pil_q[sl], settings, pilot_mode)
        cno[q] = val * 0.5 + prev * 0.5
        pld[q] = det
        prev = val
    return cno, pld


def session_cno(i_p, q_p, pil_i, pil_q, settings, pilot_mode, pieces):
    """The same values the way a session gets them: per call, the intervals that complete in it from carried + new prompts.
    Returns (list of per-call (CNo [n, 3], PLD [n, 2]), prompts still carried at the end)."""
    M = int(settings.CNoInterval)
    carry = [np.zeros(0)] * 4
    prev = np.zeros(3)
    calls, e0 = [], 0
    for k in pieces:
        new = [np.asarray(a[e0:e0 + k], dtype=np.float64) for a in (i_p, q_p, pil_i, pil_q)]
        both = [np.concatenate([c, n]) for c, n in zip(carry, new)]
        nd = len(both[0]) // M
        cno, pld = np.zeros((nd, 3)), np.zeros((nd, 2))
        for q in range(nd):
            sl = slice(q * M, (q + 1) * M)
            val, det = otrk.calc_cno_pld(both[0][sl], both[1][sl], both[2][sl], both[3][sl], settings, pilot_mode)
            cno[q] = val * 0.5 + prev * 0.5
            pld[q] = det
            prev = val
        carry = [b[nd * M:] for b in both]
        assert len(carry[0]) < M
        calls.append((cno, pld))
        e0 += k
    return calls, len(carry[0])


# ---- records ---------------------------------------------------------------------------------------------------------------
B2A_EPOCHS = 60


def _b2a_sats(spc):
    return [synth.Sat(19, 310.0, 0.37 * spc, 1.1, 47.0), synth.Sat(20, -200.0, 0.71 * spc, 0.3, 45.0),
            synth.Sat(33, 1425.0, 0.05 * spc, 2.2, 46.0)]


@functools.lru_cache(maxsize=None)
def b2a_record(iq=False):
    """The settings of BASELINE.json configs[0] (B2a, 99.375 MS/s, 1-ms epochs) with three satellites on four channels (the last
    slot unused), CNoInterval = 10, and a record of 63 code periods (6.3 MB real, 12.5 MB as I/Q pairs): 60 epochs fit with
    room, every channel meets the end of the record after 61 or 62."""
    s = bds_amd.init_settings_b2a(msToProcess=B2A_EPOCHS, numberOfChannels=4, CNoInterval=CNO_INTERVAL[B2A_EPOCHS],
                                  fileType=2 if iq else 1)
    spc = int(np.floor(s.samplingFreq / (s.codeFreqBasis / s.codeLength) + 0.5))
    sats = _b2a_sats(spc)
    x = synth.make_if(s, sats, (B2A_EPOCHS + 3) * spc, seed=77, iq_sign=-1 if iq else 0)
    chans = [SimpleNamespace(PRN=sat.prn, acquiredFreq=float(s.IF + round(sat.doppler / 25) * 25),
                             codePhase=float(int(np.ceil(sat.delay)) + 1), codeFreq=float(s.codeFreqBasis), status="T")
             for sat in sats]
    chans.append(SimpleNamespace(PRN=0, acquiredFreq=0.0, codePhase=0.0, codeFreq=0.0, status="-"))
    x.setflags(write=False)
    return s, x, chans


@functools.lru_cache(maxsize=None)
def b1c_case(mode):
    """tests/helpers.py's reduced-rate B1C case (12.5 MS/s, 10-ms epochs) cut to two channels, CNoInterval = 4, 12 epochs."""
    from helpers import track_case

    s, x, chans = track_case("B1C", mode, 12)
    x.setflags(write=False)
    return s.copy(CNoInterval=CNO_INTERVAL[12], numberOfChannels=2), x, chans[:2]
