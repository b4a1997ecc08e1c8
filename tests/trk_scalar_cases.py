"""The per-epoch scalar stage of tracking -- the loop update (apply_update) and the C/N0 + lock-detector post-pass (cno_pld_one,
k_trk_cno, k_trk_cno_seg) of csrc/bds_track.hip -- on values chosen here: the cases, and two references for each.

  *_f64   a line-by-line float64 restatement of the .m files (Calc_CNo_PLD.m; tracking.m:295-389 and the B1C counterparts through
          oracle.tracking.loop_update), sums sequential in the kernel's order, complex arithmetic where MATLAB goes complex
  *_mp    the same expressions at 50 digits (mpmath) on the same float64 inputs, with a conditioning bound for the float64 form

Shared by tests/test_trk_scalar_cases.py (CPU: the restatement lies within its bound of the 50-digit value, and every case has the
property it is named for) and tests/test_trk_scalar_gpu.py (the kernels, through the test aids bds_track_cno / bds_track_update).

What is exact and what is not.  Outputs formed by + - * / sqrt fmod alone are correctly rounded on either side and are compared bit
for bit (EXACT_UPDATE, the lock detector).  Outputs behind atan, log10 or the complex branch are compared with the 50-digit value.
The loop coefficients (calcLoopCoef, calcLoopCoefCarr, CalcWeighingFactor) are inputs of the update, not part of it: both sides
take them from the library's host helpers, which tests/test_abi_and_host.py holds to the oracle's.
"""
import functools
from collections import namedtuple
from types import SimpleNamespace

import mpmath as mp
import numpy as np

import bds_amd
from bds_amd import native
from oracle import tracking as otrk
from oracle.matlab import m_colon, m_colon_parts

import colon_states as cst

EPS = float(np.finfo(np.float64).eps)
DPS = 50
DB = 10.0 / float(np.log(10.0))  # d(10 log10 x) = DB dx / x
CODE_LEN = 10230


# =====================================================================================================================
# C/N0 and lock detector
# =====================================================================================================================
# prompts [4, n_ch, n_epochs] = I_P, Q_P, Pilot_I_P, Pilot_Q_P; done [n_ch]; pm: 0 no pilot, 1 pilot with I/Q swapped, 2 pilot as is.
# kinds {(stream, ch, q): "nan" | "+inf" | "-inf"}: the raw C/N0 of interval q of the data (stream 0) or pilot (stream 1) prompts
# that is not finite, by construction; every other interval is finite.  prop: the property the CPU test asserts.
CnoCase = namedtuple("CnoCase", "name M pm prompts done kinds prop")

# a channel at 45-48 dB-Hz: prompt amplitude over the noise of one correlator output
_SIGMA = 300.0


def cno_settings(case):
    n_ch = case.prompts.shape[1]
    if case.pm == 2:  # wide-band B1C: 10-ms epochs, pilot as is
        return bds_amd.init_settings_b1c(pilotTRKflag=2, CNoInterval=case.M, numberOfChannels=n_ch)
    return bds_amd.init_settings_b2a(pilotTRKflag=1 if case.pm else 0, CNoInterval=case.M, numberOfChannels=n_ch)


def n_cno_of(case):
    return case.prompts.shape[2] // case.M


def _noise(seed, n_ch, n_epochs):
    return np.random.default_rng(seed).normal(0.0, _SIGMA, (4, n_ch, n_epochs))


def _strong(seed, n_ch, n_epochs, pm, amp):
    """data on I_P with random symbols; the pilot where the detector looks for it: Pilot_Q_P when I/Q are swapped (pm 1), else Pilot_I_P"""
    rng = np.random.default_rng(seed)
    p = rng.normal(0.0, _SIGMA, (4, n_ch, n_epochs))
    p[0] += amp * rng.choice([-1.0, 1.0], (n_ch, n_epochs))
    p[3 if pm == 1 else 2] += 1.3 * amp
    return p


# intervals with a chosen raw value (M = 5).  I, Q of one interval:
_DZERO = (np.array([0.0, 2.0, 4.0, 6.0, 7.0]), np.zeros(5))          # Zm = 21, Zv = 441: d == 0 exactly -> lin = 0, CNo = -Inf
_CONST = (np.full(5, 3.0), np.full(5, 4.0))                          # Z = 25 throughout: Zv = 0, Nv = 0 -> +Inf
_ZERO = (np.zeros(5), np.zeros(5))                                   # 0/0 -> NaN, C/N0 and lock detector


def _put(p, stream, ch, q, iq, M=5, swapped=False):
    i, qq = iq
    a, b = (0, 1) if stream == 0 else ((3, 2) if swapped else (2, 3))  # the arrays the detector reads as I and as Q
    p[a, ch, q * M:(q + 1) * M] = i
    p[b, ch, q * M:(q + 1) * M] = qq


def _m2_case():
    """M = 2, 257 intervals: with two prompts of powers z1, z2, d = ((z1 + z2)^2 - 2 (z1 - z2)^2) / 4 is negative when z2 / z1 is below
    3 - 2 sqrt(2) = 0.17 and positive near 1.  Amplitude ratios 0.2 (power ratio 0.04: d < 0) and 0.8 (d > 0) alternate at random, 1 %
    noise on top; the last interval, the second one of thread 0, is of the first kind.  (Pure noise at M = 2 puts some of 514 intervals so
    close to d = 0 that their own rounding bound passes COND_MAX_DB.)"""
    rng = np.random.default_rng(257)
    ratio = rng.choice([0.2, 0.8], (2, 257))
    ratio[:, 256] = 0.2
    p = rng.normal(0.0, 0.01 * 2400.0, (4, 1, 514))
    for a, r in ((0, ratio[0]), (3, ratio[1])):  # data on I_P, pilot on Pilot_Q_P (swapped)
        p[a, 0, 0::2] += 2400.0
        p[a, 0, 1::2] += 2400.0 * r
    return CnoCase("m2-257-intervals-pm1", 2, 1, p, np.array([514]), {}, "second-interval")


def _special_case():
    """M = 5, pilot swapped, two channels of 9 intervals: +Inf, NaN, -Inf and -Inf followed by +Inf (the smoothing adds them: NaN), each
    between ordinary intervals, in the data stream of channel 0 and the pilot stream of channel 1"""
    p = _strong(501, 2, 45, 1, 2400.0)
    kinds = {}
    for stream, ch in ((0, 0), (1, 1)):
        for q, iq, kind in ((1, _CONST, "+inf"), (3, _ZERO, "nan"), (5, _DZERO, "-inf"), (6, _CONST, "+inf")):
            _put(p, stream, ch, q, iq, swapped=True)
            kinds[(stream, ch, q)] = kind
    return CnoCase("special-m5-smoothing", 5, 1, p, np.array([45, 45]), kinds, "special")


def _pld_case():
    """M = 5, no pilot, three channels of 2 intervals.  Channel 0: I all positive, then all negative, with sum(Q) = 0 (PLD = 1);
    channel 1: I all zero with sum(Q) != 0 (the I sums cancel: PLD = -1); channel 2: I of both signs with exact zeros (counted in
    neither sum)"""
    p = _noise(502, 3, 10)
    p[0, 0, :5] = np.abs(p[0, 0, :5]) + 1.0
    p[0, 0, 5:] = -np.abs(p[0, 0, 5:]) - 1.0
    p[1, 0] = np.array([250.0, -250.0, 125.0, -125.0, 0.0, 64.0, -32.0, -32.0, 16.0, -16.0])  # each half adds up to 0 exactly
    p[0, 1] = 0.0
    p[0, 2, [1, 3, 6]] = 0.0
    p[0, 2, [0, 5]] = -np.abs(p[0, 2, [0, 5]])
    p[0, 2, [2, 7]] = np.abs(p[0, 2, [2, 7]])
    return CnoCase("pld-edges-m5", 5, 0, p, np.array([10, 10, 10]), {}, "pld")


@functools.lru_cache(maxsize=None)
def cno_cases():
    cases = [
        # ---- strong-signal prompts: d = Zm^2 - Zv > 0, ordinary finite C/N0
        CnoCase("strong-m10-pm1", 10, 1, _strong(101, 2, 60, 1, 2400.0), np.array([60, 60]), {}, "d>0"),
        CnoCase("strong-m200-pm2", 200, 2, _strong(102, 1, 600, 2, 7000.0), np.array([600]), {}, "d>0"),
        CnoCase("strong-m50-pm0", 50, 0, _strong(103, 3, 200, 0, 2400.0), np.array([200, 200, 200]), {}, "d>0"),
        # ---- noise-only prompts (a channel on a PRN that is absent or lost): the complex branch.  Seeds chosen here, on the CPU.
        CnoCase("noise-m3-pm1", 3, 1, _noise(NOISE_SEEDS["noise-m3-pm1"], 3, 120), np.array([120] * 3), {}, "noise"),
        CnoCase("noise-m10-pm0", 10, 0, _noise(NOISE_SEEDS["noise-m10-pm0"], 2, 200), np.array([200] * 2), {}, "noise"),
        CnoCase("noise-m50-pm2", 50, 2, _noise(NOISE_SEEDS["noise-m50-pm2"], 2, 500), np.array([500] * 2), {}, "noise"),
        CnoCase("noise-m200-pm2", 200, 2, _noise(NOISE_SEEDS["noise-m200-pm2"], 2, 1200), np.array([1200] * 2), {}, "noise"),
        # 257 intervals of M = 2: one workgroup of 256 threads per channel, so thread 0 takes a second interval
        _m2_case(),
        # ---- exact edges
        _special_case(),
        _pld_case(),
        # ---- channels whose `done` ends inside an interval (37 = 3 intervals + 7; 9 = none) or before the arrays end
        CnoCase("done-mid-interval-m10", 10, 1, _strong(104, 3, 50, 1, 2400.0), np.array([50, 37, 9]), {}, "done"),
    ]
    for c in cases:
        c.prompts.setflags(write=False)
    return tuple(cases)


# seeds of the noise cases: the first seed from 1 on for which at least a third of the intervals of the data stream have d < 0 and
# every interval's conditioning bound (cno_bound_db) is below COND_MAX_DB -- both are properties of the inputs alone (CPU)
NOISE_SEEDS = {"noise-m3-pm1": 1, "noise-m10-pm0": 1, "noise-m50-pm2": 1, "noise-m200-pm2": 6}
# C/N0 near d = 0 is ill-conditioned (lin ~ sqrt|d|): a case whose own rounding bound reached the 1e-9 dB budget could not tell a
# kernel error from its inputs.  Every finite output of every case stays a factor of four below it.
COND_MAX_DB = 2.5e-10


def piece_lists(n_epochs, M):
    """Two cuts of n_epochs into pieces.  The first has every interval boundary strictly inside a piece (edges at M // 2 + k M); the
    second mixes pieces of 1, M - 1, M + 1 and 2 M - 1 epochs, so that edges also fall ON boundaries and calls complete 0, 1 or 2
    intervals."""
    a = [max(1, M // 2)]
    while sum(a) < n_epochs:
        a.append(min(M, n_epochs - sum(a)))
    b, cyc, i = [], (1, M - 1, M + 1, 2 * M - 1), 0
    while sum(b) < n_epochs:
        b.append(min(cyc[i % 4], n_epochs - sum(b)))
        i += 1
    return [a, b]


def cno_one_f64(I, Q, M, T):
    """Calc_CNo_PLD.m for one channel component over M prompts, float64, the sums sequential as cno_pld_one runs them.
    Returns (d, lin, cno, pld)."""
    I = np.asarray(I, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    T = np.float64(T)
    with np.errstate(all="ignore"):
        zm = np.float64(0.0)
        for i in range(M):
            zm = zm + (I[i] * I[i] + Q[i] * Q[i])  # Z = I_P.^2 + Q_P.^2; Zm = mean(Z)
        zm = zm / M
        zv = np.float64(0.0)
        for i in range(M):
            z = I[i] * I[i] + Q[i] * Q[i]
            zv = zv + (z - zm) * (z - zm)
        zv = zv / (M - 1)  # Zv = var(Z)
        d = zm * zm - zv
        if d < 0:  # Pav = sqrt(Zm^2 - Zv) is complex: MATLAB's sqrt of a negative real is 1i * sqrt(-x)
            pav = complex(0.0, float(np.sqrt(-d)))
            nv = 0.5 * (complex(float(zm), 0.0) - pav)  # Nv = 0.5 * (Zm - Pav)
            lin = np.float64(abs((1 / float(T)) * pav / (2 * nv)))  # abs((1/T) * Pav / (2 * Nv))
        else:
            pav = np.sqrt(d)
            nv = 0.5 * (zm - pav)
            lin = np.abs((1 / T) * pav / (2 * nv))
        cno = 10 * np.log10(lin)
        sp = sn = sq = np.float64(0.0)
        for i in range(M):
            if I[i] > 0:
                sp = sp + I[i]
            if I[i] < 0:
                sn = sn + I[i]
            sq = sq + Q[i]
        a = (sp - sn) * (sp - sn)  # NBP / NBD
        pld = (a - sq * sq) / (a + sq * sq)
    return float(d), float(lin), float(cno), float(pld)


def _streams(case, ch, q):
    """(I, Q) the detector reads for the data and for the pilot of interval q (Calc_CNo_PLD.m: the narrow-band / B2a variant swaps)"""
    sl = slice(q * case.M, (q + 1) * case.M)
    p = case.prompts
    out = [(p[0, ch, sl], p[1, ch, sl])]
    if case.pm == 2:
        out.append((p[2, ch, sl], p[3, ch, sl]))
    elif case.pm == 1:
        out.append((p[3, ch, sl], p[2, ch, sl]))
    return out


def _series(case, one, add, log10, half_sum, zero):
    """The post-pass over a case with the arithmetic of `one` & co: cno5 as nested lists [5][n_ch][n_cno] (tracking.m:411-434: raw
    values, then CNo = new/2 + previous/2 with previous = 0 before the first interval)."""
    n_ch, n_cno, T = case.prompts.shape[1], n_cno_of(case), cno_settings(case).intTime
    out = [[[zero] * n_cno for _ in range(n_ch)] for _ in range(5)]
    per = {}
    for ch in range(n_ch):
        prev = [zero] * 3
        for q in range(int(case.done[ch]) // case.M):
            res = [one(i, qq, case.M, T) for i, qq in _streams(case, ch, q)]
            per[(ch, q)] = res
            raw = [res[0]["cno"], res[1]["cno"] if case.pm else zero, log10(add(res[0]["lin"], res[1]["lin"] if case.pm else zero))]
            out[0][ch][q] = half_sum(raw[0], prev[0])
            out[1][ch][q] = res[0]["pld"]
            if case.pm:
                out[2][ch][q] = half_sum(raw[1], prev[1])
                out[3][ch][q] = res[1]["pld"]
                out[4][ch][q] = half_sum(raw[2], prev[2])
            prev = raw
    return out, per


@functools.lru_cache(maxsize=None)
def cno_f64(name):
    """(cno5 [5, n_ch, n_cno] float64 restatement, d [2, n_ch, n_cno] of the data / pilot stream, NaN where not evaluated)"""
    case = cno_case(name)

    def one(i, q, M, T):
        d, lin, cno, pld = cno_one_f64(i, q, M, T)
        return dict(d=d, lin=np.float64(lin), cno=np.float64(cno), pld=np.float64(pld))

    with np.errstate(all="ignore"):
        out, per = _series(case, one, lambda a, b: a + b, lambda v: 10 * np.log10(v), lambda a, b: a * 0.5 + b * 0.5, np.float64(0.0))
    d = np.full((2, case.prompts.shape[1], n_cno_of(case)), np.nan)
    for (ch, q), res in per.items():
        for st, r in enumerate(res):
            d[st, ch, q] = r["d"]
    return np.array(out, dtype=np.float64), d


def cno_case(name):
    return {c.name: c for c in cno_cases()}[name]


# ---- 50 digits ------------------------------------------------------------------------------------------------------
def _mp_log10(v):
    if mp.isnan(v):
        return mp.nan
    if v == 0:
        return mp.mpf("-inf")
    if v == mp.inf:
        return mp.inf
    return 10 * mp.log10(v)


def _mp_add(a, b):
    return a + b


def cno_one_mp(I, Q, M, T):
    """The same expressions at 50 digits on the float64 prompts.  `rel`: a bound on the relative error of the float64 form's lin.

    The bound, for sums of M terms in float64 (u = EPS / 2 per operation, written with EPS to have a margin of two):
      Zm            sum of M non-negative terms of two products and an add each: relative error <= (M + 3) EPS
      Zv            each term (z - Zm)^2 carries 2 (M + 4) EPS Zm |z - Zm|; by Cauchy-Schwarz over the M terms and the division by M - 1
                    the sum carries <= 2 sqrt(2) (M + 4) EPS Zm sqrt(Zv), plus (M + 2) EPS Zv of its own
      d = Zm^2 - Zv absolute error <= (M + 4) EPS (2 Zm^2 + 2 sqrt(2) Zm sqrt(Zv) + Zv) <= 2 (M + 4) EPS (Zm + sqrt(Zv))^2 =: ed
      sqrt|d|       relative error rs = ed / (2 |d|) + EPS
      d < 0         lin = (s / T) / hypot(Zm, s): rs + max((M + 3) EPS, rs) + 4 EPS
      d >= 0        Nv = (Zm - Pav) / 2 cancels: relative error rn = ((M + 3) EPS Zm + Pav rs) / (Zm - Pav) + EPS; lin: rs + rn + 4 EPS
    """
    with mp.workdps(DPS):
        I = [mp.mpf(float(v)) for v in I]
        Q = [mp.mpf(float(v)) for v in Q]
        T = mp.mpf(float(T))
        z = [i * i + q * q for i, q in zip(I, Q)]
        zm = mp.fsum(z) / M
        zv = mp.fsum((v - zm) ** 2 for v in z) / (M - 1)
        d = zm * zm - zv
        ed = 2 * (M + 4) * EPS * (zm + mp.sqrt(zv)) ** 2
        rel = mp.mpf(0)
        if zm == 0:
            lin = mp.nan  # 0 / 0
        elif d < 0:
            s = mp.sqrt(-d)
            lin = (s / T) / mp.sqrt(zm * zm + s * s)
            rs = ed / (2 * -d) + EPS
            rel = rs + max((M + 3) * EPS, rs) + 4 * EPS
        else:
            pav = mp.sqrt(d)
            nv = (zm - pav) / 2
            if nv == 0:
                lin = mp.inf
            elif d == 0:
                lin = mp.mpf(0)
            else:
                lin = abs((1 / T) * pav / (2 * nv))
                rs = ed / (2 * d) + EPS
                rel = rs + ((M + 3) * EPS * zm + pav * rs) / (zm - pav) + EPS + 4 * EPS
        cno = _mp_log10(lin)
        sp = mp.fsum(v for v in I if v > 0)
        sn = mp.fsum(v for v in I if v < 0)
        sq = mp.fsum(Q)
        a = (sp - sn) ** 2
        pld = mp.nan if a + sq * sq == 0 else (a - sq * sq) / (a + sq * sq)
        return dict(d=d, lin=lin, cno=cno, pld=pld, rel=rel)


@functools.lru_cache(maxsize=None)
def cno_mp(name):
    """(cno5 [5, n_ch, n_cno] of the 50-digit evaluation rounded to float64, bound [5, n_ch, n_cno]: what the float64 form may differ
    from it by: in dB for the C/N0 rows (0, 2, 4), absolute for the lock-detector rows (1, 3), which lie within [-1, 1])"""
    case = cno_case(name)
    with mp.workdps(DPS):
        def half(a, b):
            if mp.isnan(a) or mp.isnan(b) or (mp.isinf(a) and mp.isinf(b) and a != b):
                return mp.nan
            return a / 2 + b / 2

        def add(a, b):
            return mp.nan if mp.isnan(a) or mp.isnan(b) else a + b

        out, per = _series(case, cno_one_mp, add, _mp_log10, half, mp.mpf(0))
        n_ch, n_cno = case.prompts.shape[1], n_cno_of(case)
        bound = np.zeros((5, n_ch, n_cno))

        def fin(v):
            return float(abs(v)) if mp.isfinite(v) else 0.0

        for ch in range(n_ch):
            praw = [0.0, 0.0, 0.0]
            pval = [0.0, 0.0, 0.0]
            for q in range(int(case.done[ch]) // case.M):
                res = per[(ch, q)]
                rels = [float(r["rel"]) for r in res] + [0.0]
                lin_sum = add(res[0]["lin"], res[1]["lin"] if case.pm else mp.mpf(0))
                val = [fin(res[0]["cno"]), fin(res[1]["cno"]) if case.pm else 0.0, fin(_mp_log10(lin_sum))]
                raw = [DB * rels[0] + 4 * EPS * val[0], DB * rels[1] + 4 * EPS * val[1], DB * (max(rels[0], rels[1]) + EPS) + 4 * EPS * val[2]]
                for row, j in ((0, 0), (2, 1), (4, 2)):
                    bound[row, ch, q] = 0.5 * (raw[j] + praw[j]) + EPS * (val[j] + pval[j])
                praw, pval = raw, val
        bound[[1, 3]] = (case.M + 6) * EPS  # sums of M terms, two squares, a quotient within [-1, 1]
        return np.array([[[float(v) for v in r] for r in plane] for plane in out]), bound


def cno_expected_masks(case):
    """(nan, +inf, -inf) masks [5, n_ch, n_cno] of cno5 that follow from case.kinds alone: a raw NaN or Inf reaches its own interval
    and, through the two-point smoothing, the next one (+Inf/2 + -Inf/2 = NaN); only an all-zero interval makes the lock detector NaN"""
    n_ch, n_cno = case.prompts.shape[1], n_cno_of(case)
    m = {k: np.zeros((5, n_ch, n_cno), dtype=bool) for k in ("nan", "+inf", "-inf")}

    def join_lin(a, b):  # of dlin + plin: lin kinds are NaN, +Inf, 0 (written "-inf") or finite ("")
        if "nan" in (a, b):
            return "nan"
        if "+inf" in (a, b):
            return "+inf"
        return "-inf" if a == b == "-inf" else ""

    def smooth(a, b):
        if "nan" in (a, b) or {a, b} == {"+inf", "-inf"}:
            return "nan"
        return a or b

    for ch in range(n_ch):
        prev = ["", "", ""]
        for q in range(int(case.done[ch]) // case.M):
            kd, kp = case.kinds.get((0, ch, q), ""), case.kinds.get((1, ch, q), "")
            raw = [kd, kp, join_lin(kd, kp)]
            rows = ((0, 0), (2, 1), (4, 2)) if case.pm else ((0, 0),)
            for row, j in rows:
                k = smooth(raw[j], prev[j])
                if k:
                    m[k][row, ch, q] = True
            if kd == "nan":
                m["nan"][1, ch, q] = True
            if case.pm and kp == "nan":
                m["nan"][3, ch, q] = True
            prev = raw
    return m["nan"], m["+inf"], m["-inf"]


# =====================================================================================================================
# the loop update
# =====================================================================================================================
STATE = native.UPDATE_STATE
NEXT = [f + "'" for f in STATE]
# outputs behind atan: compared with the 50-digit value.  Every other output is formed by + - * / sqrt fmod alone: bit for bit.
MP_UPDATE = ("pllDiscr", "pllDiscrFilt", "carrFreq'", "d2CarrError'", "dCarrError'")
EPOCH_FIELDS = native.TRACK_FIELDS[:21]
EXACT_UPDATE = tuple(f for f in NEXT + EPOCH_FIELDS if f not in MP_UPDATE)

UpdRow = namedtuple("UpdRow", "name state sums stop nan")   # nan: the outputs that are NaN, by construction; stop: active' == 0
UpdCfg = namedtuple("UpdCfg", "name mode pilot settings rows")

_PLL_NAN = frozenset(MP_UPDATE)
_DLL_NAN = frozenset(("dllDiscr", "dllDiscrFilt", "codeFreq'", "oldCodeNco'", "oldCodeError'"))


def _base_state(signal, s):
    nominal = 10.23e6 if signal == "B2A" else 1.023e6
    return dict(codeFreq=nominal + 3.2, remCodePhase=0.123, carrFreq=s.IF + 1234.5, carrFreqBasis=s.IF + 1200.0, remCarrPhase=1.234,
                oldCodeNco=0.8, oldCodeError=0.01, d2CarrError=30.0, dCarrError=25.0, codeFreqBasis=nominal)


#                        I_E       Q_E      I_P      Q_P      I_L      Q_L
_BASE_SUMS = np.array([15210.5, 1310.25, 30100.75, 2520.5, 14890.25, 1190.75,       # data
                       -1150.5, 16870.25, -2210.75, 33420.5, -1290.25, 16410.75,    # pilot BOC(1,1) / B2a pilot
                       410.25, -2110.5, 820.75, -4330.25, 395.5, -2080.75])         # pilot BOC(6,1)


def _rows(signal, mode, pilot, s):
    base = _base_state(signal, s)

    def row(name, stop=False, nan=(), sums=None, **state):
        st = dict(base)
        st.update(state)
        sm = _BASE_SUMS.copy()
        for k, v in (sums or {}).items():
            sm[k] = v
        return UpdRow(name, np.array([st[f] for f in STATE]), sm, stop, frozenset(nan))

    rows = [
        row("typical"),
        # atan(Q_P / I_P) with true division: I_P = 0 gives +-pi/2 by the sign of Q_P.  The update adds the partial sums up from +0,
        # so a -0 partial sum reaches the discriminator as +0: all four are +-1/4 cycle by the sign of Q_P alone.
        row("ip+0-q+", sums={2: 0.0, 3: 5.0}), row("ip-0-q+", sums={2: -0.0, 3: 5.0}),
        row("ip+0-q-", sums={2: 0.0, 3: -5.0}), row("ip-0-q-", sums={2: -0.0, 3: -5.0}),
        row("ip-neg", sums={2: -30100.75}),  # atan, not atan2: the half-plane of I_P is not seen
        row("pll-0/0", nan=_PLL_NAN, sums={2: 0.0, 3: 0.0}),  # NaN carrier loop; the code loop goes on
        row("e=l", sums={0: 14890.25, 1: 1190.75, 6: -1290.25, 7: 16410.75, 12: 395.5, 13: -2080.75}),
        row("e+l=0", stop=True, nan=_DLL_NAN, sums={k: 0.0 for k in (0, 1, 4, 5)}),  # 0/0 in the DLL: no next block
        row("zero-sums", stop=True, nan=_PLL_NAN | _DLL_NAN, sums={k: 0.0 for k in range(18)}),  # an epoch of all-zero samples
        row("codefreq<=0", stop=True, oldCodeNco=2.0e7),  # finite everywhere, but the code NCO leaves the positive numbers
        row("trig-negative", carrFreq=-(s.IF + 77.7), remCarrPhase=-3.0),
        row("trig-large", carrFreq=1.5e9 + 0.7, remCarrPhase=6.2),
        row("rem-negative", remCodePhase=-0.37),
    ]
    if pilot:
        # the pilot discriminator's denominator at 0.  B2a: QI = (pI + j pQ) exp(-j pi/2), and cos(-pi/2) is 6.1e-17, not 0: with
        # pQ_P = 0 the real part is pI 6.1e-17 and atan(imag / real) is finite division; NB: atan(-pI / 0); WB: the composite's I
        # is -sqrt(4/33) sI_P + sqrt(29/33) pQ_P, 0 when both are
        rows.append(row("pilot-denominator-0", sums={9: 0.0, 14: 0.0}))
        rows.append(row("pilot-numerator-0", sums={8: 0.0, 15: 0.0}))
    return rows


def _colon_rows():
    """one configuration per distinct (signal, mode, fs, spacing, rem, code rate) of tests/colon_states.py: the states on which MATLAB's
    colon vector is not a + k d (and the quiet ones), at the block tracking itself takes"""
    seen, out = set(), []
    for st in list(cst.STATES) + list(cst.QUIET):
        key = (st.signal, st.mode, st.fs, st.spacing, st.rem, st.code_freq)
        if key in seen:
            continue
        seen.add(key)
        s = cst.settings_of(st, n_ch=1)
        state = _base_state(st.signal, s)
        state.update(codeFreq=st.code_freq or cst.nominal_code_freq(st.signal), remCodePhase=st.rem)
        r = UpdRow(st.name, np.array([state[f] for f in STATE]), _BASE_SUMS.copy(), False, frozenset())
        out.append(UpdCfg("colon-" + st.name, st.mode, True, s, (r,)))
    return out


@functools.lru_cache(maxsize=None)
def update_cfgs():
    """B2a, narrow-band and wide-band B1C, with the pilot on and off.  (Wide-band mode IS pilotTRKflag == 2: it has no pilot-off
    variant; with the flag at 0 B1C runs the narrow-band tracker without pilot.)"""
    out = []
    for name, signal, mode, flag in (("b2a-pilot", "B2A", "B2A", 1), ("b2a-data", "B2A", "B2A", 0), ("nb-pilot", "B1C", "NB", 1),
                                     ("nb-data", "B1C", "NB", 0), ("wb-pilot", "B1C", "WB", 2)):
        if signal == "B2A":
            s = bds_amd.init_settings_b2a(samplingFreq=25e6, IF=6.5e6, pilotTRKflag=flag)
        else:
            s = bds_amd.init_settings_b1c(samplingFreq=12.5e6, IF=3.5e6, pilotTRKflag=flag, FEBW=10e6)
        pilot = flag != 0
        rows = tuple(_rows(signal, mode, pilot, s))
        out.append(UpdCfg(name, mode, pilot, s.copy(numberOfChannels=len(rows)), rows))
    return tuple(out) + tuple(_colon_rows())


def update_cfg(name):
    return {c.name: c for c in update_cfgs()}[name]


@functools.lru_cache(maxsize=None)
def _coef(cfg_name):
    """the loop coefficients as the library's host helpers give them to the kernel (fill_params)"""
    s = update_cfg(cfg_name).settings
    tau1, tau2 = native.calc_loop_coef(s.dllNoiseBandwidth, s.dllDampingRatio, 1.0)
    pf3, pf2, pf1 = native.calc_loop_coef_carr(s)
    factor = native.calc_weighing_factor(s) if update_cfg(cfg_name).mode == "WB" else 0.0
    return SimpleNamespace(pf3=pf3, pf2=pf2, pf1=pf1, tau1=tau1, tau2=tau2, pdi=s.intTime, spc_el=s.dllCorrelatorSpacing, factor=factor)


def tp_last_of(cfg, row):
    """(last element of the prompt colon vector tcode as MATLAB builds it, blk): tracking.m:260-263 / NB_tracking.m:271-273"""
    st = dict(zip(STATE, row.state))
    step = st["codeFreq"] / cfg.settings.samplingFreq  # :230
    blk = int(np.ceil((CODE_LEN - st["remCodePhase"]) / step))  # :233
    sc = 1.0 if cfg.mode == "B2A" else 2.0
    t_p = m_colon(st["remCodePhase"] * sc, step * sc, ((blk - 1) * step + st["remCodePhase"]) * sc)
    assert len(t_p) == blk, (cfg.name, row.name, len(t_p), blk)
    return float(t_p[-1]), blk, step


def update_f64(cfg, row):
    """The epoch's outputs and the next state, float64, line by line: dict over NEXT + EPOCH_FIELDS + active', completed'."""
    s, mode, b2a = cfg.settings, cfg.mode, cfg.mode == "B2A"
    st = dict(zip(STATE, (np.float64(v) for v in row.state)))
    sums = np.float64(0.0) + np.asarray(row.sums, dtype=np.float64)  # the fixed-order sum of the partial sums starts from +0
    data6, p11, p61 = tuple(sums[0:6]), tuple(sums[6:12]), tuple(sums[12:18])
    pil6 = None
    if cfg.pilot:
        pil6 = otrk.qmboc_composite(p11, p61) if mode == "WB" else p11
    tp_last, blk, step = tp_last_of(cfg, row)
    step = np.float64(step)
    with np.errstate(all="ignore"):
        rem_next = (np.float64(tp_last) + step) - CODE_LEN if b2a else np.float64(tp_last) / 2 + step - CODE_LEN  # :295 / WB:327
        t_end = np.float64(blk) / np.float64(s.samplingFreq)  # time(blksize+1), :303
        trig_end = ((st["carrFreq"] * 2.0 * np.pi) * t_end) + st["remCarrPhase"]  # :304
        carr_next = np.fmod(trig_end, 2.0 * np.pi)  # :305
    up = otrk.loop_update(mode, cfg.pilot, data6, pil6,
                          SimpleNamespace(d2=st["d2CarrError"], d1=st["dCarrError"], old_nco=st["oldCodeNco"], old_err=st["oldCodeError"],
                                          carr_basis=st["carrFreqBasis"], code_basis=st["codeFreqBasis"]), _coef(cfg.name))
    out = {f: 0.0 for f in EPOCH_FIELDS}  # the template's zeros where the tracker writes nothing (pilot fields without pilot)
    out.update(absoluteSample=0.0, codeFreq=st["codeFreq"], carrFreq=st["carrFreq"], remCodePhase=st["remCodePhase"],
               remCarrPhase=st["remCarrPhase"], dllDiscr=up.code_err, dllDiscrFilt=up.code_nco, pllDiscr=up.carr_err, pllDiscrFilt=up.carr_nco)
    for f, v in zip(("I_E", "Q_E", "I_P", "Q_P", "I_L", "Q_L"), data6):
        out[f] = v
    if cfg.pilot:
        if mode == "WB":
            for f, v in zip(("Pilot_I_E", "Pilot_Q_E", "Pilot_I_P", "Pilot_Q_P", "Pilot_I_L", "Pilot_Q_L"), pil6):
                out[f] = v
        else:
            out["Pilot_I_P"], out["Pilot_Q_P"] = p11[2], p11[3]
    out.update({"codeFreq'": up.code_freq, "remCodePhase'": rem_next, "carrFreq'": up.carr_freq, "carrFreqBasis'": st["carrFreqBasis"],
                "remCarrPhase'": carr_next, "oldCodeNco'": up.code_nco, "oldCodeError'": up.code_err, "d2CarrError'": up.d2,
                "dCarrError'": up.d1, "codeFreqBasis'": st["codeFreqBasis"]})
    out = {k: float(v) for k, v in out.items()}
    out["active'"] = 1 if otrk.nco_state_ok(out["codeFreq'"], out["remCodePhase'"]) else 0
    out["completed'"] = 1
    return out


def update_mp(cfg, row):
    """The same expressions at 50 digits on the same float64 inputs: (value, scale) dicts over the outputs the update computes.
    `scale` is the sum of the magnitudes that enter an output; the float64 form may differ from the value by UPDATE_OPS EPS scale."""
    s, mode, b2a = cfg.settings, cfg.mode, cfg.mode == "B2A"
    co = _coef(cfg.name)
    with mp.workdps(DPS):
        F = lambda v: mp.mpf(float(v))  # noqa: E731
        st = {f: F(v) for f, v in zip(STATE, row.state)}
        sums = [F(0.0 + float(v)) for v in row.sums]
        two_pi, L = F(2.0 * np.pi), CODE_LEN

        def div(a, b):  # true division by a +0 denominator
            if mp.isnan(a) or mp.isnan(b):
                return mp.nan
            if b == 0:
                return mp.nan if a == 0 else (mp.inf if a > 0 else -mp.inf)
            return a / b

        def atan_div(a, b):
            q = div(a, b)
            return mp.nan if mp.isnan(q) else mp.atan(q) / two_pi

        d6, p11, p61 = sums[0:6], sums[6:12], sums[12:18]
        pil = None
        if cfg.pilot:
            if mode == "WB":
                a, b = mp.sqrt(F(4) / 33), mp.sqrt(F(29) / 33)
                pil = [-a * p61[0] + b * p11[1], -a * p61[1] - b * p11[0], -a * p61[2] + b * p11[3], -a * p61[3] - b * p11[2],
                       -a * p61[4] + b * p11[5], -a * p61[5] - b * p11[4]]
            else:
                pil = p11
        ce = atan_div(d6[3], d6[2])
        s_ce = abs(ce)
        if cfg.pilot:
            if b2a:
                rot = np.exp(-1j * np.pi / 2)  # as MATLAB evaluates it: the float64 pair (6.1e-17, -1)
                cr, sr = F(rot.real), F(rot.imag)
                cq = atan_div(pil[2] * sr + pil[3] * cr, pil[2] * cr - pil[3] * sr)
                ce, s_ce = (ce + cq) / 2, (abs(ce) + abs(cq)) / 2
            elif mode == "NB":
                cq = atan_div(-pil[2], pil[3])
                ce, s_ce = (ce * 11 + cq * 29) / 40, (abs(ce) * 11 + abs(cq) * 29) / 40
            else:
                cq = atan_div(pil[3], pil[2])
                ce, s_ce = (ce + cq * 3) / 4, (abs(ce) + abs(cq) * 3) / 4
        pf3, pf2, pf1 = F(co.pf3), F(co.pf2), F(co.pf1)
        d2 = st["d2CarrError"] + ce * pf3
        s_d2 = abs(st["d2CarrError"]) + s_ce * pf3
        d1 = d2 + ce * pf2 + st["dCarrError"]
        s_d1 = s_d2 + s_ce * pf2 + abs(st["dCarrError"])
        nco = d1 + ce * pf1
        s_nco = s_d1 + s_ce * pf1
        carr = st["carrFreqBasis"] + nco
        s_carr = abs(st["carrFreqBasis"]) + s_nco

        def env(a, b):
            return mp.sqrt(a * a + b * b)

        def el(v):
            e, l = env(v[0], v[1]), env(v[4], v[5])
            return div(e - l, e + l)

        spc = F(co.spc_el)
        cd = el(d6)
        s_cd = mp.mpf(1)  # |(E - L) / (E + L)| <= 1, and the difference E - L carries EPS (E + L)
        if not b2a:
            cd, s_cd = cd * (1 - spc), s_cd * (1 - spc)
        if cfg.pilot:
            pce = el(pil)
            if b2a:
                cd, s_cd = (cd + pce) / 2, (s_cd + 1) / 2
            elif mode == "NB":
                cd, s_cd = (cd * 11 + pce * (1 - spc) * 29) / 40, (s_cd * 11 + (1 - spc) * 29) / 40
            else:
                fa = F(co.factor)
                cd, s_cd = cd * fa + pce * (1 - spc) * (1 - fa), s_cd * fa + (1 - spc) * (1 - fa)
        tau1, tau2, pdi = F(co.tau1), F(co.tau2), F(co.pdi)
        cn = st["oldCodeNco"] + (tau2 / tau1) * (cd - st["oldCodeError"]) + cd * (pdi / tau1)
        s_cn = abs(st["oldCodeNco"]) + (tau2 / tau1) * (s_cd + abs(st["oldCodeError"])) + s_cd * (pdi / tau1)
        cf = st["codeFreqBasis"] - cn
        s_cf = abs(st["codeFreqBasis"]) + s_cn
        tp_last, blk, step = tp_last_of(cfg, row)
        step_mp = st["codeFreq"] / F(s.samplingFreq)
        tp = (st["remCodePhase"] + (blk - 1) * step_mp)  # the colon vector's last element, exactly
        rem_next = tp + step_mp - L
        trig = st["carrFreq"] * two_pi * (F(blk) / F(s.samplingFreq)) + st["remCarrPhase"]
        k = mp.floor(abs(trig) / two_pi)
        carr_next = trig - mp.sign(trig) * k * two_pi  # rem(x, 2*pi): the sign of x
        val = {"pllDiscr": ce, "pllDiscrFilt": nco, "carrFreq'": carr, "d2CarrError'": d2, "dCarrError'": d1,
               "dllDiscr": cd, "dllDiscrFilt": cn, "codeFreq'": cf, "oldCodeNco'": cn, "oldCodeError'": cd,
               "remCodePhase'": rem_next, "remCarrPhase'": carr_next}
        scale = {"pllDiscr": s_ce, "pllDiscrFilt": s_nco, "carrFreq'": s_carr, "d2CarrError'": s_d2, "dCarrError'": s_d1,
                 "dllDiscr": s_cd, "dllDiscrFilt": s_cn, "codeFreq'": s_cf, "oldCodeNco'": s_cn, "oldCodeError'": s_cd,
                 "remCodePhase'": mp.mpf(2 * L), "remCarrPhase'": abs(trig) + two_pi}
        if cfg.pilot and mode == "WB":
            for f, v, i, j in zip(("Pilot_I_E", "Pilot_Q_E", "Pilot_I_P", "Pilot_Q_P", "Pilot_I_L", "Pilot_Q_L"), pil, (0, 1, 2, 3, 4, 5), (1, 0, 3, 2, 5, 4)):
                val[f], scale[f] = v, abs(p61[i]) + abs(p11[j])
        return ({k: (float("nan") if mp.isnan(v) else float(v)) for k, v in val.items()}, {k: float(v) for k, v in scale.items()},
                {k: v for k, v in val.items()})


# rounding steps of half an EPS each between the inputs and any output of the update, relative to the output's scale: the quotient, atan,
# the division by 2 pi, the weighted mean of two discriminators (3), three filter stages of a product and a sum each, the basis: 16
# steps, 8 EPS
UPDATE_OPS = 8


def update_error(name, got, ref, scale):
    """|got - ref| / scale of one output, `ref` the unrounded 50-digit value (third result of update_mp): the rounding of the output
    itself is part of the figure, so a correctly rounded output does not read as 0.  inf when only one of the two is finite."""
    with mp.workdps(DPS):
        ref = mp.mpf(ref)
        if not (np.isfinite(got) and mp.isfinite(ref)):
            return 0.0 if (np.isnan(got) and mp.isnan(ref)) or (np.isinf(got) and mp.mpf(got) == ref) else float("inf")
        if mp.mpf(got) == ref:
            return 0.0
        return float("inf") if scale == 0 else float(abs(mp.mpf(got) - ref) / scale)


def colon_scan(n=4000, seed=7):
    """Random code NCO states around the trackers' rates: (rem + (blk-1) step [*2 ...] as the update forms it) and the colon vector's
    right-hand end point c, for ADVICE item 1.  Returns the number of states where they differ and where n != blk - 1."""
    rng = np.random.default_rng(seed)
    differ = short = 0
    for i in range(n):
        b2a = bool(i & 1)
        fs = rng.choice([12.5e6, 25e6, 30.69e6, 53e6, 61.38e6, 99.375e6, 102.3e6])
        step = (10.23e6 if b2a else 1.023e6) * (1 + rng.uniform(-2e-2, 2e-2)) / fs
        rem = float(rng.choice([0.0, rng.uniform(-0.5, 0.999), round(rng.uniform(0, 1), 2)]))
        blk = int(np.ceil((CODE_LEN - rem) / step))
        sc = 1.0 if b2a else 2.0
        nn, c = m_colon_parts(rem * sc, step * sc, ((blk - 1) * step + rem) * sc)
        kernel = rem + (blk - 1) * step if b2a else rem * 2.0 + (blk - 1) * (step * 2.0)
        short += nn != blk - 1
        differ += kernel != c
    return differ, short


# =====================================================================================================================
# end to end: a channel on a PRN that is not in the record
# =====================================================================================================================
ABSENT_PRN = 40
E2E_SEED = {"b2a": 21, "b1c-wb": 21}   # helpers.track_case's seed; see e2e_negative_intervals
E2E_MIN_NEGATIVE = {"b2a": 3, "b1c-wb": 2}


@functools.lru_cache(maxsize=None)
def e2e_case(which):
    """(settings, record, channels, mode).  b2a: helpers.track_case("B2A", "B2A", 60) with CNoInterval = 5; b1c-wb: the wide-band case of
    track_session_cases.b1c_case (12 epochs, CNoInterval = 4, two channels); in both the last channel is moved to ABSENT_PRN."""
    from helpers import track_case
    from track_session_cases import CNO_INTERVAL

    if which == "b2a":
        s, x, chans = track_case("B2A", "B2A", 60, seed=E2E_SEED[which])
        s, mode = s.copy(CNoInterval=5), "B2A"
    else:
        s, x, chans = track_case("B1C", "WB", 12, seed=E2E_SEED[which])
        s, chans, mode = s.copy(CNoInterval=CNO_INTERVAL[12], numberOfChannels=2), chans[:2], "WB"
    chans = [SimpleNamespace(**vars(c)) for c in chans]
    chans[-1].PRN = ABSENT_PRN
    x.setflags(write=False)
    return s, x, tuple(chans), mode


@functools.lru_cache(maxsize=None)
def e2e_oracle(which):
    s, x, chans, mode = e2e_case(which)
    ref, _ = otrk.tracking(otrk.RawFile(x), list(chans), s, mode=mode)
    return ref


def e2e_negative_intervals(which):
    """intervals of the moved channel, in the oracle's own run, whose data or pilot prompts have d = Zm^2 - Zv < 0"""
    s, _, chans, mode = e2e_case(which)
    r = e2e_oracle(which)[len(chans) - 1]
    M = int(s.CNoInterval)
    n = 0
    for q in range(len(r.I_P) // M):
        sl = slice(q * M, (q + 1) * M)
        pil = (r.Pilot_I_P[sl], r.Pilot_Q_P[sl]) if mode == "WB" else (r.Pilot_Q_P[sl], r.Pilot_I_P[sl])
        n += any(cno_one_f64(i, qq, M, s.intTime)[0] < 0 for i, qq in ((r.I_P[sl], r.Q_P[sl]), pil))
    return n


@functools.lru_cache(maxsize=None)
def zero_stretch_case():
    """helpers.track_case("B2A", "B2A", 8) with every sample zero from the start of the first channel's third epoch on: that epoch
    correlates to exact zeros, atan(0/0) and 0/0 make the next code rate NaN, and the run stops there as at a short read"""
    from helpers import track_case

    s, x, chans = track_case("B2A", "B2A", 8)
    s = s.copy(CNoInterval=2)
    clean, _ = otrk.tracking(otrk.RawFile(x), chans, s, mode="B2A")
    x = x.copy()
    x[int(clean[0].absoluteSample[2]):] = 0
    x.setflags(write=False)
    return s, x, tuple(chans)
