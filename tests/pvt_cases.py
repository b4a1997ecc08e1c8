"""Position fix: a float64 / NumPy restatement of the reference's postNavigation chain, and the builder of the scenarios the
tests feed to bds_pvt_plan / bds_pvt_measure / bds_pvt_solve / bds_post_navigation.  Test infrastructure only; nothing here is
loaded by the library.

Restated, with the reference's line numbers (B1C and B2a files are equal where one is named):
    BDS-3_B1C/postNavigation.m:69-298 (readiness: :82; BDS-3_B2a/postNavigation.m:84-85)
    Common/calculatePseudoranges.m:63-110
    BDS-3_B1C/include/satpos.m:32-153, include/check_t.m:19-27
    Common/leastSquarePos.m:33-121, Common/e_r_corr.m:21-32, include/topocent.m:24-56, Common/togeod.m:32-111,
    Common/tropo.m:34-97, Common/cart2geo.m:22-51

`Model` holds the choices at which a restatement can silently go wrong; the defaults are the reference's, and
tests/test_pvt_cases.py shows that each other setting is caught.

The scenario builder makes the three tracking series of every channel from a receiver position and ephemerides: for each code
period k it finds when the period that left the satellite at TOW + (k - subFrameStart) T arrives (the restatement's own satpos,
the rotation of e_r_corr, no troposphere) and writes absoluteSample = ceil(s_k), remCodePhase = (ceil(s_k) - s_k) codeFreq / fs
and codeFreq = codeLength / (arrival of k + 1 - arrival of k) = codeFreqBasis (1 - rangeRate / c).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace
from types import SimpleNamespace

import numpy as np

# ---- the reference's constants (pinned by tests/golden/pvt_constants.json) -------------------------------------------------------
BDS_PI = 3.1415926535898            # satpos.m:32
OMEGA_E = 7.2921150e-5              # :34
MU = 3.986004418e14                 # :35
F_REL = -4.44280730904398e-10       # :37
A_REF_MEO = 27906100                # :38
A_REF_IGSO_GEO = 42162200           # :39
OMEGAE_DOT = 7.292115147e-5         # e_r_corr.m:21
ELL5_A, ELL5_FINV = 6378137, 298.257223563  # cart2geo.m:22-23, entry 5
TOPO_A, TOPO_FINV = 6378137.0, 298.257222101  # topocent.m:26
TROPO = {"a_e": 6378.137, "b0": 7.839257e-5, "tlapse": -6.5}  # tropo.m:34-36
TROPO_ARGS = (0.0, 1013.0, 293.0, 50.0, 0.0, 0.0, 0.0)  # leastSquarePos.m:71
HALF_WEEK = 302400                  # check_t.m:19
READY, IDLE, NO_EPH, NO_SATTYPE, NO_FRAME = 1, 2, 4, 8, 16  # BDS_PVT_* (include/bds_mi355x.h)
GEO, IGSO, MEO = 1, 2, 3            # bds_eph.SatType


@dataclass(frozen=True)
class Model:
    e_r_corr: bool = True       # leastSquarePos.m:63 rotates the satellite by the travel time
    index_ge: bool = False      # calculatePseudoranges.m:77 with >= in place of >
    index_minus1: bool = True   # :82
    tgd_sign: float = -1.0      # satpos.m:61,151: T_GDB1Cp is subtracted
    sfs_offset: int = 0         # calculatePseudoranges.m:96: subFrameStart as given
    check_t: bool = True        # satpos.m:54,67
    dt1_zero: bool = True       # postNavigation.m:218-219


REFERENCE = Model()


# ---- satpos ----------------------------------------------------------------------------------------------------------------------
def check_t(t, model=REFERENCE):
    """check_t.m:19-27, element-wise."""
    t = np.asarray(t)
    if not model.check_t:
        return t
    return np.where(t > HALF_WEEK, t - 2 * HALF_WEEK, np.where(t < -HALF_WEEK, t + 2 * HALF_WEEK, t))


def satpos(transmit_time, e, b1c, model=REFERENCE, dtype=np.float64, trace=None):
    """satpos.m:54-151 for one ephemeris (a dict of bds_eph's names) at an array of transmit times -> (pos [..., 3], clk [...]).
    `dtype` np.longdouble gives the same formulas in extended precision; `trace`, a dict, receives Phi, tk and dt."""
    f = dtype
    t = np.asarray(transmit_time, dtype=f)
    g = {k: f(v) for k, v in e.items() if isinstance(v, float)}
    two_pi = 2 * f(BDS_PI)
    tgd = model.tgd_sign * g["T_GDB1Cp"] if b1c else f(0.0)  # B2a: the term is 0 (the library's rule)
    dt = check_t(t - g["t_oc"], model).astype(f)                                  # :54
    clk0 = (g["a_2"] * dt + g["a_1"]) * dt + g["a_0"] + tgd                       # :59-61
    time = t - clk0                                                               # :63
    tk = check_t(time - g["t_oe"], model).astype(f)                               # :67
    A_ref = f(A_REF_MEO) if e["SatType"] == MEO else f(A_REF_IGSO_GEO)            # :69-73
    A0 = A_ref + g["deltaA"]                                                      # :76
    A = A0 + g["ADot"] * tk                                                       # :77
    n0 = np.sqrt(f(MU) / (A0 * A0 * A0))                                          # :80
    delta_n = g["delta_n_0"] + f(0.5) * g["delta_n_0Dot"] * tk                    # :81
    n = n0 + delta_n                                                              # :84
    M = g["M_0"] + n * tk                                                         # :87
    M = np.fmod(M + two_pi, two_pi)                                               # :90
    E = np.array(M, dtype=f, copy=True)
    live = np.ones(E.shape, dtype=bool)                                           # the loop breaks per element (:101-104)
    for _ in range(10):                                                           # :96-105
        E_new = M + g["e"] * np.sin(E)
        dE = np.fmod(E_new - E, two_pi)
        E = np.where(live, E_new, E)
        live = live & ~(np.abs(dE) < 1.e-12)
        if not live.any():
            break
    E = np.fmod(E + two_pi, two_pi)                                               # :108
    dtr = f(F_REL) * g["e"] * np.sqrt(A0) * np.sin(E)                             # :111
    nu = np.arctan2(np.sqrt(1 - g["e"] * g["e"]) * np.sin(E), np.cos(E) - g["e"])  # :114
    Phi = np.fmod(nu + g["omega"], two_pi)                                        # :117-120
    c2, s2 = np.cos(2 * Phi), np.sin(2 * Phi)
    u = Phi + g["C_uc"] * c2 + g["C_us"] * s2                                     # :123-125
    r = A * (1 - g["e"] * np.cos(E)) + g["C_rc"] * c2 + g["C_rs"] * s2            # :127-129
    i = g["i_0"] + g["i_0Dot"] * tk + g["C_ic"] * c2 + g["C_is"] * s2             # :131-133
    Omega = g["omega_0"] + (g["omegaDot"] - f(OMEGA_E)) * tk - f(OMEGA_E) * g["t_oe"]  # :136-137
    Omega = np.fmod(Omega + two_pi, two_pi)                                       # :139
    xp, yp = r * np.cos(u), r * np.sin(u)                                         # :142-143
    pos = np.stack([xp * np.cos(Omega) - yp * np.cos(i) * np.sin(Omega),          # :144-146
                    xp * np.sin(Omega) + yp * np.cos(i) * np.cos(Omega),
                    yp * np.sin(i)], axis=-1)
    clk = (g["a_2"] * dt + g["a_1"]) * dt + g["a_0"] + tgd + dtr                  # :150-151
    if trace is not None:
        trace.update(Phi=Phi, tk=tk, dt=dt, raw_tk=time - g["t_oe"])
    return pos, clk


# ---- calculatePseudoranges -------------------------------------------------------------------------------------------------------
def index_scan(abs_sample, sample, start=1):
    """calculatePseudoranges.m:76-82 as written: the loop variable at the break (or at the end of the range), minus 1."""
    index = start
    for index in range(start, len(abs_sample) + 1):
        if abs_sample[index - 1] > sample:
            break
    return index - 1


def index_search(abs_sample, samples, model=REFERENCE):
    """The same by bisection, for an array of samples (what the kernel does): the first entry strictly greater, clipped to n, - 1."""
    ub = np.searchsorted(abs_sample, samples, side="left" if model.index_ge else "right")
    return np.minimum(ub + 1, len(abs_sample)) - (1 if model.index_minus1 else 0)


def transmit_time(settings, abs_sample, code_freq, rem_code_phase, index, samples, sub_frame_start, tow, model=REFERENCE):
    """calculatePseudoranges.m:85-97, `index` 1-based."""
    k = np.asarray(index) - 1
    step = code_freq[k] / settings.samplingFreq
    code_phase = rem_code_phase[k] + step * (samples - abs_sample[k])
    L = float(settings.codeLength)
    return ((code_phase / L + np.asarray(index, dtype=np.float64)) - (sub_frame_start + model.sfs_offset)) * L / settings.codeFreqBasis + tow


def measure(settings, ready, abs_sample, code_freq, rem_code_phase, ephs, sub_frame_start, tow, sample_start, step, n_meas,
            model=REFERENCE):
    """The measurement stage: (transmitTime [n_meas, n_ch], satPos [n_meas, n_ch, 3], satClkCorr [n_meas, n_ch], index [n_meas, n_ch]);
    NaN (index 0) on a channel that is not ready."""
    b1c = str(settings.signal).upper() == "B1C"
    n_ch = len(ready)
    tt, sp, ck = np.full((n_meas, n_ch), np.nan), np.full((n_meas, n_ch, 3), np.nan), np.full((n_meas, n_ch), np.nan)
    idx = np.zeros((n_meas, n_ch), dtype=np.int64)
    samples = sample_start + step * np.arange(n_meas, dtype=np.float64)  # postNavigation.m:172
    for c in range(n_ch):
        if not ready[c] & READY:
            continue
        idx[:, c] = index_search(abs_sample[c], samples, model)
        tt[:, c] = transmit_time(settings, abs_sample[c], code_freq[c], rem_code_phase[c], idx[:, c], samples, sub_frame_start[c], tow[c], model)
        sp[:, c], ck[:, c] = satpos(tt[:, c], ephs[c], b1c, model)
    return tt, sp, ck, idx


# ---- leastSquarePos and what it calls ----------------------------------------------------------------------------------------------
def e_r_corr(traveltime, x):
    """e_r_corr.m:21-32."""
    w = OMEGAE_DOT * traveltime
    R3 = np.array([[math.cos(w), math.sin(w), 0], [-math.sin(w), math.cos(w), 0], [0, 0, 1]])
    return R3 @ x


def togeod(a, finv, X, Y, Z):
    """togeod.m:32-111 -> (dphi [deg], dlambda [deg], h)."""
    h, tolsq, maxit = 0.0, 1.e-10, 10
    rtd = 180 / math.pi
    esq = 0.0 if finv < 1.e-20 else (2 - 1 / finv) / finv
    oneesq = 1 - esq
    P = math.sqrt(X * X + Y * Y)
    dlambda = math.atan2(Y, X) * rtd if P > 1.e-20 else 0.0
    if dlambda < 0:
        dlambda = dlambda + 360
    r = math.sqrt(P * P + Z * Z)
    sinphi = Z / r if r > 1.e-20 else 0.0
    dphi = math.asin(sinphi)
    if r < 1.e-20:
        return dphi, dlambda, 0.0
    h = r - a * (1 - sinphi * sinphi / finv)
    for _ in range(maxit):
        sinphi, cosphi = math.sin(dphi), math.cos(dphi)
        N_phi = a / math.sqrt(1 - esq * sinphi * sinphi)
        dP = P - (N_phi + h) * cosphi
        dZ = Z - (N_phi * oneesq + h) * sinphi
        h = h + (sinphi * dZ + cosphi * dP)
        dphi = dphi + (cosphi * dZ - sinphi * dP) / (N_phi + h)
        if dP * dP + dZ * dZ < tolsq:
            break
    return dphi * rtd, dlambda, h


def topocent(X, dx):
    """topocent.m:24-54 -> (Az, El) [deg]."""
    dtr = math.pi / 180
    phi, lam, _ = togeod(TOPO_A, TOPO_FINV, X[0], X[1], X[2])
    cl, sl, cb, sb = math.cos(lam * dtr), math.sin(lam * dtr), math.cos(phi * dtr), math.sin(phi * dtr)
    Fm = np.array([[-sl, -sb * cl, cb * cl], [cl, -sb * sl, cb * sl], [0, cb, sb]])
    E, N, U = Fm.T @ np.asarray(dx, dtype=np.float64)
    hor_dis = math.sqrt(E * E + N * N)
    if hor_dis < 1.e-20:
        Az, El = 0.0, 90.0
    else:
        Az, El = math.atan2(E, N) / dtr, math.atan2(U, hor_dis) / dtr
    if Az < 0:
        Az = Az + 360
    return Az, El


def tropo(sinel, hsta, p, tkel, hum, hp, htkel, hhum):
    """tropo.m:34-97."""
    a_e, b0, tlapse = TROPO["a_e"], TROPO["b0"], TROPO["tlapse"]
    tkhum = tkel + tlapse * (hhum - htkel)
    atkel = 7.5 * (tkhum - 273.15) / (237.3 + tkhum - 273.15)
    e0 = 0.0611 * hum * 10 ** atkel
    tksea = tkel - tlapse * htkel
    em = -978.77 / (2.8704e6 * tlapse * 1.0e-5)
    tkelh = tksea + tlapse * hhum
    e0sea = e0 * (tksea / tkelh) ** (4 * em)
    tkelp = tksea + tlapse * hp
    psea = p * (tksea / tkelp) ** em
    if sinel < 0:
        sinel = 0.0
    trop = 0.0
    refsea = 77.624e-6 / tksea
    htop = 1.1385e-5 / refsea
    refsea = refsea * psea
    ref = refsea * ((htop - hsta) / htop) ** 4
    for done in (False, True):
        rtop = (a_e + htop) ** 2 - (a_e + hsta) ** 2 * (1 - sinel ** 2)
        if rtop < 0:
            rtop = 0.0
        rtop = math.sqrt(rtop) - (a_e + hsta) * sinel
        a = -sinel / (htop - hsta)
        b = -b0 * (1 - sinel ** 2) / (htop - hsta)
        rn = np.array([rtop ** (i + 1) for i in range(1, 9)])
        alpha = np.array([2 * a, 2 * a ** 2 + 4 * b / 3, a * (a ** 2 + 3 * b), a ** 4 / 5 + 2.4 * a ** 2 * b + 1.2 * b ** 2,
                          2 * a * b * (a ** 2 + 3 * b) / 3, b ** 2 * (6 * a ** 2 + 4 * b) * 1.428571e-1, 0, 0])
        if b ** 2 > 1.0e-35:
            alpha[6], alpha[7] = a * b ** 3 / 2, b ** 4 / 9
        dr = rtop + float(alpha @ rn)
        trop = trop + dr * ref * 1000
        if done:
            break
        refsea = (371900.0e-6 / tksea - 12.92e-6) / tksea
        htop = 1.1385e-5 * (1255 / tksea + 0.05) / refsea
        ref = refsea * e0sea * ((htop - hsta) / htop) ** 4
    return trop


def cart2geo5(X, Y, Z):
    """cart2geo.m:22-51 with i = 5 -> (phi [deg], lambda [deg], h).  (0, 0, 0) gives NaN, 0, NaN as in MATLAB."""
    with np.errstate(all="ignore"):
        X, Y, Z = np.float64(X), np.float64(Y), np.float64(Z)
        a, f = np.float64(ELL5_A), 1 / np.float64(ELL5_FINV)
        lam = np.arctan2(Y, X)
        ex2 = (2 - f) * f / ((1 - f) ** 2)
        c = a * np.sqrt(1 + ex2)
        P = np.sqrt(X ** 2 + Y ** 2)
        phi = np.arctan(Z / ((P * (1 - (2 - f))) * f))
        h, oldh, iterations = np.float64(0.1), np.float64(0), 0
        while abs(h - oldh) > 1.e-12:
            oldh = h
            N = c / np.sqrt(1 + ex2 * np.cos(phi) ** 2)
            phi = np.arctan(Z / (P * (1 - (2 - f) * f * N / (N + h))))
            h = P / np.cos(phi) - N
            iterations += 1
            if iterations > 100:
                break
        return float(phi * 180 / np.pi), float(lam * 180 / np.pi), float(h)


def matlab_rank(A):
    """rank(A): singular values above max(size(A)) * eps(max(s)); a matrix with NaN / inf, at which MATLAB stops, has rank 0 here."""
    if not np.isfinite(A).all():
        return 0
    s = np.linalg.svd(A, compute_uv=False)
    return int((s > max(A.shape) * np.spacing(s.max())).sum())


def least_square_pos(sat_pos, obs, settings, model=REFERENCE):
    """leastSquarePos.m:33-121: satpos [ns, 3], obs [ns] -> (pos [4], el [ns], az [ns], dop [5], A of the last iteration)."""
    dtr = math.pi / 180
    ns = len(obs)
    pos = np.zeros(4)
    A, omc = np.zeros((ns, 4)), np.zeros(ns)
    az, el = np.zeros(ns), np.zeros(ns)
    for it in range(1, 11):
        for i in range(ns):
            X = sat_pos[i]
            if it == 1:
                Rot_X, trop = X.copy(), 2.0
            else:
                rho2 = (X[0] - pos[0]) ** 2 + (X[1] - pos[1]) ** 2 + (X[2] - pos[2]) ** 2
                traveltime = math.sqrt(rho2) / settings.c
                Rot_X = e_r_corr(traveltime, X) if model.e_r_corr else X.copy()
                az[i], el[i] = topocent(pos[:3], Rot_X - pos[:3])
                trop = tropo(math.sin(el[i] * dtr), *TROPO_ARGS) if settings.useTropCorr == 1 else 0.0
            d = Rot_X - pos[:3]
            nrm = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            omc[i] = obs[i] - nrm - pos[3] - trop
            A[i] = [-d[0] / nrm, -d[1] / nrm, -d[2] / nrm, 1]
        if matlab_rank(A) != 4:
            return np.zeros(4), el, az, np.full(5, np.inf), A
        pos = pos + np.linalg.lstsq(A, omc, rcond=None)[0]
    Q = np.linalg.inv(A.T @ A)
    dop = np.array([math.sqrt(np.trace(Q)), math.sqrt(Q[0, 0] + Q[1, 1] + Q[2, 2]), math.sqrt(Q[0, 0] + Q[1, 1]),
                    math.sqrt(Q[2, 2]), math.sqrt(Q[3, 3])])
    return pos, el, az, dop, A


# ---- postNavigation --------------------------------------------------------------------------------------------------------------
def is_ready(e, b1c):
    if e is None:
        return False
    if b1c:
        return e["flag"] == 1  # BDS-3_B1C/postNavigation.m:82
    iv = list(e["idValid"])
    return iv[0] == 10 and iv[1] == 11 and any(iv[2 + k] == 30 + k for k in range(5))  # BDS-3_B2a/postNavigation.m:84-85


def plan(settings, status, abs_sample, ephs, sub_frame_start, tow):
    """postNavigation.m:69-122 with the library's own drops -> the dict native.pvt_plan gives."""
    b1c = str(settings.signal).upper() == "B1C"
    n_ch, n = abs_sample.shape
    ready = np.zeros(n_ch, dtype=np.int32)
    for c in range(n_ch):
        f = sub_frame_start[c]
        if status[c] == "-":
            ready[c] = IDLE
        elif not is_ready(ephs[c], b1c):
            ready[c] = NO_EPH
        elif ephs[c]["SatType"] not in (GEO, IGSO, MEO):
            ready[c] = NO_SATTYPE
        elif not (1 <= f <= n and f == math.floor(f)) or not math.isfinite(tow[c]):
            ready[c] = NO_FRAME
        else:
            ready[c] = READY
    step = float(math.trunc(settings.samplingFreq * settings.navSolPeriod / 1000))  # :119
    out = {"ready": ready, "sampleStart": math.nan, "sampleEnd": math.nan, "measSampleStep": step, "n_meas": 0}
    on = np.nonzero(ready & READY)[0]
    if on.size < 4:  # :92
        return out
    out["sampleStart"] = max(0.0, max(abs_sample[c, int(sub_frame_start[c]) - 1] for c in on)) + 1  # :103-115
    out["sampleEnd"] = min(abs_sample[c, -1] for c in on) - 1  # :110,116
    out["n_meas"] = max(0, math.trunc((out["sampleEnd"] - out["sampleStart"]) / step))  # :122
    return out


def solve(settings, prns, ready, sample_start, step, tt_all, sp_all, ck_all, model=REFERENCE):
    """postNavigation.m:146-298 over the measurement stage's arrays -> the arrays of navSolutions by name, plus "active" (the
    list per epoch) and "A" (the last matrix of each fix, None without one)."""
    n_meas, n_ch = tt_all.shape
    o = {f: np.zeros((n_ch, n_meas)) for f in ("PRN", "correctedP")}
    o.update((f, np.full((n_ch, n_meas), np.nan)) for f in ("el", "az", "transmitTime", "satClkCorr"))
    o["rawP"] = np.zeros((n_ch, n_meas))
    o["DOP"] = np.zeros((5, n_meas))
    o.update((f, np.full(n_meas, np.nan)) for f in ("X", "Y", "Z", "dt", "localTime", "currMeasSample", "latitude", "longitude", "height"))
    o["active"], o["A"] = [], []
    satElev = np.full(n_ch, np.inf)  # :129
    localTime = math.inf             # :139
    with np.errstate(invalid="ignore"):
        for m in range(n_meas):
            active = [c for c in range(n_ch) if ready[c] & READY and satElev[c] >= settings.elevationMask]  # :151-152
            o["active"].append(active)
            o["PRN"][active, m] = [prns[c] for c in active]  # :155-156
            cms = sample_start + step * m  # :172
            tt = np.full(n_ch, np.inf)  # calculatePseudoranges.m:64
            tt[active] = tt_all[m, active]
            if localTime == math.inf:  # :102-105
                localTime = (np.nanmax(tt[active]) if np.isfinite(tt[active]).any() else math.nan) + settings.startOffset / 1000
            rawP = (localTime - tt) * settings.c  # :110
            o["rawP"][:, m] = rawP
            o["transmitTime"][active, m] = tt[active]  # :182-183
            clk = ck_all[m, active]
            o["satClkCorr"][active, m] = clk  # :192
            if len(active) > 3:  # :197
                obs = rawP[active] + clk * settings.c  # :201-202
                pos, el, az, dop, A = least_square_pos(sp_all[m, active], obs, settings, model)
                o["A"].append(A)
                o["el"][active, m], o["az"][active, m], o["DOP"][:, m] = el, az, dop
                o["X"][m], o["Y"][m], o["Z"][m] = pos[:3]  # :212-214
                o["dt"][m] = 0 if (m == 0 and model.dt1_zero) else pos[3]  # :218-222
                localTime = localTime - pos[3] / settings.c  # :225
                o["localTime"][m], o["currMeasSample"][m] = localTime, cms
                satElev = o["el"][:, m].copy()  # :232
                o["correctedP"][active, m] = rawP[active] + clk * settings.c - pos[3]  # :235-237
                o["latitude"][m], o["longitude"][m], o["height"][m] = cart2geo5(pos[0], pos[1], pos[2])  # :242-248
            else:
                o["A"].append(None)  # :270-285: X .. height NaN (as initialised), DOP zeros
            localTime = localTime + step / settings.samplingFreq  # :296
    return o


# ---- ephemerides and scenarios -----------------------------------------------------------------------------------------------------
def geodetic_to_ecef(lat_deg, lon_deg, h):
    a, f = 6378137.0, 1 / 298.257223563
    e2 = f * (2 - f)
    lat, lon = math.radians(lat_deg), math.radians(lon_deg)
    N = a / math.sqrt(1 - e2 * math.sin(lat) ** 2)
    return np.array([(N + h) * math.cos(lat) * math.cos(lon), (N + h) * math.cos(lat) * math.sin(lon), (N * (1 - e2) + h) * math.sin(lat)])


def _semicircles(rad, bits):
    """A signed raw integer of `bits` bits for an angle [rad] in a field scaled 2^-(bits - 1) * pi."""
    v = round((math.remainder(rad, 2 * math.pi) / BDS_PI) * (1 << (bits - 1)))
    return max(-(1 << (bits - 1)), min((1 << (bits - 1)) - 1, v))


def orbit_fields(rx, az_deg, el_deg, sat_type, ecc, t_ref, t_oe, rng):
    """Raw integers of the orbit fields (names of synth.BCNAV1_FIELDS / BCNAV2_FIELDS) for a satellite that, at system time t_ref, is seen
    from `rx` near azimuth `az_deg`, elevation `el_deg` (exact for a circular orbit; the tests measure what comes out)."""
    lat, lon = math.atan2(rx[2], math.hypot(rx[0], rx[1])), math.atan2(rx[1], rx[0])
    east = np.array([-math.sin(lon), math.cos(lon), 0.0])
    north = np.array([-math.sin(lat) * math.cos(lon), -math.sin(lat) * math.sin(lon), math.cos(lat)])
    up = np.array([math.cos(lat) * math.cos(lon), math.cos(lat) * math.sin(lon), math.sin(lat)])
    az, el = math.radians(az_deg), math.radians(el_deg)
    d = math.cos(el) * (math.sin(az) * east + math.cos(az) * north) + math.sin(el) * up
    r = float(A_REF_MEO if sat_type == MEO else A_REF_IGSO_GEO)
    b = float(rx @ d)
    rho = -b + math.sqrt(b * b - float(rx @ rx) + r * r)  # |rx + rho d| = r
    p = rx + rho * d
    lat_s, lon_s = math.asin(p[2] / r), math.atan2(p[1], p[0])
    inc = max(math.radians(55.0), abs(lat_s) + math.radians(5.0))
    u = math.asin(math.sin(lat_s) / math.sin(inc))
    Omega = lon_s - math.atan2(math.sin(u) * math.cos(inc), math.cos(u))  # node longitude in the rotating frame at t_ref
    n0 = math.sqrt(MU / r ** 3)
    tk = float(check_t(t_ref - t_oe))  # what satpos will take as the time from the ephemeris epoch
    omega = float(rng.uniform(-3.0, 3.0))
    f = {"t_oe": t_oe // 300, "SatType": sat_type, "deltaA": int(rng.integers(-2000, 2000)), "ADot": int(rng.integers(-200, 200)),
         "delta_n_0": int(rng.integers(-2000, 2000)), "delta_n_0Dot": int(rng.integers(-2000, 2000)),
         "M_0": _semicircles(u - omega - n0 * tk, 33), "e": int(round(ecc * 2 ** 34)), "omega": _semicircles(omega, 33),
         "omega_0": _semicircles(Omega + OMEGA_E * (tk + t_oe), 33), "i_0": _semicircles(inc, 33),
         "omegaDot": int(rng.integers(-3000, 0)), "i_0Dot": int(rng.integers(-300, 300))}
    for name in ("C_is", "C_ic", "C_us", "C_uc"):
        f[name] = int(rng.integers(-3000, 3000))   # 2^-30 rad: a few microradians
    for name in ("C_rs", "C_rc"):
        f[name] = int(rng.integers(-60000, 60000))  # 2^-8 m: a few hundred metres
    return f


def clock_fields(t_oc, rng):
    return {"t_oc": t_oc // 300, "a_0": int(rng.integers(-(1 << 22), 1 << 22)), "a_1": int(rng.integers(-(1 << 14), 1 << 14)),
            "a_2": int(rng.integers(-200, 200))}


def make_eph(signal, prn, tow, orbit, clock, rng):
    """(the ephemeris as native.nav_fields parses it back, the messages' bits [n_msg, 878 / 288], the raw fields per message)."""
    from bds_amd import native, synth

    import nav_cases as nc

    if signal == "B1C":
        assert tow % 18 == 0 and 0 <= tow < 255 * 3600
        f = dict(PRN=prn, SOH=(tow % 3600) // 18, HOW=tow // 3600, WN=int(rng.integers(0, 8192)), PageID=1, **orbit, **clock,
                 T_GDB1Cp=int(rng.integers(-2000, 2000)), T_GDB2ap=int(rng.integers(-2000, 2000)), ISC_B1Cd=int(rng.integers(-2000, 2000)))
        bits = synth.pack_bcnav1_fields(**f)
        bits[590:614] = nc.crc_bits(bits[14:590])
        bits[854:878] = nc.crc_bits(bits[614:854])
        msgs, raw = bits[None], [f]
    else:
        assert tow % 3 == 0
        names10 = ("t_oe", "SatType", "deltaA", "ADot", "delta_n_0", "delta_n_0Dot", "M_0", "e", "omega")
        raw = [dict(MesType=10, PRN=prn, SOW=tow // 3, WN=int(rng.integers(0, 8192)), **{k: orbit[k] for k in names10}),
               dict(MesType=11, PRN=prn, SOW=tow // 3 + 1, **{k: v for k, v in orbit.items() if k not in names10}),
               dict(MesType=30, PRN=prn, SOW=tow // 3 + 2, **clock)]
        msgs = []
        for f in raw:
            b = synth.pack_bcnav2_fields(**f)
            msgs.append(np.concatenate([b, nc.crc_bits(b)]))
        msgs = np.stack(msgs)
    e, entered = native.nav_fields(signal, msgs)
    assert entered == len(msgs)
    return e, msgs, raw


def default_sky(n_ch):
    """(azimuth, elevation, SatType, eccentricity) per channel: spread in azimuth, 15 .. 80 degrees up, MEO and IGSO, e = 0 and 0.02."""
    return [((37.0 + 360.0 * c / n_ch + 11.0 * (c % 3)) % 360.0, 15.0 + (c * 23) % 66, MEO if c % 3 else IGSO, 0.02 if c % 2 else 0.0)
            for c in range(n_ch)]


def make_scenario(signal, n_ch, n, rx=None, sky=None, tow=7218, clk_rx=1.234e-4, seed=1, t_oe=None, prns=None, lead=0, overrides=None):
    """A consistent set of tracking series and ephemerides.  `sky` as default_sky gives; `clk_rx` moves the sampling grid against
    system time; `lead` code periods stand before the earliest arrival of the frame."""
    import bds_amd

    rng = np.random.default_rng(seed)
    settings = (bds_amd.init_settings_b1c if signal == "B1C" else bds_amd.init_settings_b2a)(numberOfChannels=n_ch, **(overrides or {}))
    b1c = signal == "B1C"
    rx = geodetic_to_ecef(39.9, 116.4, 57.0) if rx is None else np.asarray(rx, dtype=np.float64)
    sky = default_sky(n_ch) if sky is None else sky
    prns = [19 + c for c in range(n_ch)] if prns is None else prns
    t_oe = (tow // 300) * 300 if t_oe is None else t_oe
    T = settings.codeLength / settings.codeFreqBasis
    fs, c_light = settings.samplingFreq, float(settings.c)
    t0 = 0.060 - lead * T + clk_rx  # system time of sample 0, relative to tow
    ephs, msgs, raws = [], [], []
    abs_sample, code_freq, rem = np.zeros((n_ch, n)), np.zeros((n_ch, n)), np.zeros((n_ch, n))
    sfs = np.zeros(n_ch)
    for c in range(n_ch):
        az, el, sat_type, ecc = sky[c]
        e, m, raw = make_eph(signal, prns[c], tow, orbit_fields(rx, az, el, sat_type, ecc, tow + 0.1, t_oe, rng), clock_fields(t_oe, rng), rng)
        ephs.append(e), msgs.append(m), raws.append(raw)

        def delay(rel):  # arrival minus satellite-clock time of departure, for departures tow + rel
            pos, clk = satpos(tow + rel, e, b1c)
            travel = np.sqrt(((pos - rx) ** 2).sum(axis=-1)) / c_light
            w = OMEGAE_DOT * travel
            rot = np.stack([np.cos(w) * pos[..., 0] + np.sin(w) * pos[..., 1], -np.sin(w) * pos[..., 0] + np.cos(w) * pos[..., 1],
                            pos[..., 2]], axis=-1)  # e_r_corr
            return np.sqrt(((rot - rx) ** 2).sum(axis=-1)) / c_light - clk

        first = int(math.floor((float(delay(np.float64(0.0))) - t0) / T)) + 1  # the period in which the frame arrives
        assert first >= 1
        sfs[c] = first
        rel = (np.arange(1, n + 2) - first) * T  # departures of periods 1 .. n + 1, relative to tow
        arrive = (rel - t0) + delay(rel)         # system time of arrival relative to sample 0 (small numbers: no week-second rounding)
        s = arrive * fs
        abs_sample[c] = np.ceil(s[:n])
        code_freq[c] = settings.codeLength / (arrive[1:] - arrive[:-1])
        rem[c] = (abs_sample[c] - s[:n]) * code_freq[c] / fs
        assert abs_sample[c, 0] >= 0
    return SimpleNamespace(signal=signal, settings=settings, rx=rx, tow=tow, t0=t0, prns=np.array(prns, dtype=np.int32), ephs=ephs, msgs=msgs,
                           raws=raws, status="T" * n_ch, absoluteSample=abs_sample, codeFreq=code_freq, remCodePhase=rem,
                           subFrameStart=sfs, TOW=np.full(n_ch, float(tow)), n_ch=n_ch, n=n)


def run_reference(scn, model=REFERENCE, settings=None, n_meas=None):
    """plan -> measure -> solve of the restatement on a scenario: (plan dict, (tt, sp, ck, idx), solve dict or None)."""
    s = settings or scn.settings
    p = plan(s, scn.status, scn.absoluteSample, scn.ephs, scn.subFrameStart, scn.TOW)
    nm = p["n_meas"] if n_meas is None else min(n_meas, p["n_meas"])
    if nm <= 0:
        return p, None, None
    meas = measure(s, p["ready"], scn.absoluteSample, scn.codeFreq, scn.remCodePhase, scn.ephs, scn.subFrameStart, scn.TOW,
                   p["sampleStart"], p["measSampleStep"], nm, model)
    return p, meas, solve(s, scn.prns, p["ready"], p["sampleStart"], p["measSampleStep"], *meas[:3], model)


def truth_bound(A, tow, c_light):
    """|fix - truth| <= ||pinv(A)||_2 sqrt(n_sat) (2 ulp(TOW) c + 1e-4 m): seconds-of-week rounding and the range acceleration
    ignored within one code period."""
    smin = np.linalg.svd(A, compute_uv=False).min()
    return (1 / smin) * math.sqrt(A.shape[0]) * (2 * float(np.spacing(np.float64(tow))) * c_light + 1e-4)


# ---- comparing a solution with the restatement's ------------------------------------------------------------------------------------
# Quantity: tolerance and where it comes from.
#   transmitTime                     bit-equal: only IEEE + - * /
#   satClkCorr                       1e-16 s: its ulp is ~1e-20 s
#   X, Y, Z, height, correctedP      1e-5 m: cond(A) <= 50 times a few ulp(2.6e7 m) ~ 1e-6 m, 10x margin
#   latitude, longitude, el, az      1e-9 deg: from the X, Y, Z bound
#   DOP                              relative 1e-9
#   dt, rawP                         1e-5 m + 2 ulp(localTime) c: a sub-micrometre difference in dt can round localTime - dt / c to
#   localTime                        2 ulp     the neighbouring double, which moves every later raw pseudorange and dt by the same
#                                              ~9 mm and leaves the position and correctedP untouched
ABS_TOL = {"satClkCorr": 1e-16, "X": 1e-5, "Y": 1e-5, "Z": 1e-5, "height": 1e-5, "correctedP": 1e-5,
           "latitude": 1e-9, "longitude": 1e-9, "el": 1e-9, "az": 1e-9}
SOLUTION_FIELDS = ["PRN", "el", "az", "transmitTime", "satClkCorr", "rawP", "correctedP", "DOP", "X", "Y", "Z", "dt", "localTime",
                   "currMeasSample", "latitude", "longitude", "height"]


def compare_solutions(got, want, c_light=299792458.0):
    """Assert the table above on two sets of navSolutions arrays; returns the worst difference per quantity."""
    worst = {}
    for f in SOLUTION_FIELDS:
        g, w = np.asarray(got[f], dtype=np.float64), np.asarray(want[f], dtype=np.float64)
        assert g.shape == w.shape, (f, g.shape, w.shape)
        # the NaN / +-inf / 0 places are identical
        assert np.array_equal(np.isnan(g), np.isnan(w)), f
        inf = np.isinf(w)
        assert np.array_equal(np.isinf(g), inf) and np.array_equal(g[inf], w[inf]), f
        assert np.array_equal(g == 0, w == 0), f
        fin = np.isfinite(w)
        d = np.abs(np.where(fin, g, 0) - np.where(fin, w, 0))
        if f in ("PRN", "currMeasSample", "transmitTime"):
            tol = 0.0
        elif f == "DOP":
            d = d / np.where(fin & (w != 0), np.abs(w), 1.0)
            tol = 1e-9
        elif f in ("dt", "rawP", "localTime"):
            lt = np.where(np.isfinite(want["localTime"]), want["localTime"], np.nanmax(np.abs(want["transmitTime"])) + 0.1)
            ulp = np.spacing(np.abs(lt))
            tol = 2 * ulp if f == "localTime" else 1e-5 + 2 * ulp * c_light  # per epoch; broadcasts over the channels of rawP
        else:
            tol = ABS_TOL[f]
        worst[f] = float(d.max()) if d.size else 0.0
        assert (d <= tol).all(), (f, worst[f], np.max(tol))
    return worst


def copy_channel(scn, src, dst):
    """Channel `dst` becomes a second row of channel `src`: the same PRN, ephemeris and series."""
    for a in (scn.absoluteSample, scn.codeFreq, scn.remCodePhase, scn.subFrameStart, scn.TOW, scn.prns):
        a[dst] = a[src]
    scn.ephs[dst], scn.msgs[dst], scn.raws[dst] = scn.ephs[src], scn.msgs[src], scn.raws[src]


def sky_with(n_ch, low=None):
    """default_sky with channel `low` at 3 degrees of elevation (below the 5 degree mask)."""
    sky = default_sky(n_ch)
    if low is not None:
        sky[low] = (sky[low][0], 3.0, MEO, 0.0)
    return sky


def host_cases():
    """name -> scenario for the chain tests (tests/test_pvt_host.py on the restatement's measurement arrays, tests/test_pvt_gpu.py
    through bds_post_navigation).  Built once per process."""
    if not _HOST_CASES:
        fast = dict(navSolPeriod=50)
        c = _HOST_CASES
        c["b1c_5x7"] = make_scenario("B1C", 5, 48, overrides=fast, seed=11)
        c["b1c_5x7_notrop"] = make_scenario("B1C", 5, 48, overrides=dict(fast, useTropCorr=0), seed=11)
        c["b1c_4x1"] = make_scenario("B1C", 4, 40, seed=12)
        c["low_of_5"] = make_scenario("B1C", 5, 40, sky=sky_with(5, low=2), overrides=fast, seed=13)
        c["low_of_4"] = make_scenario("B1C", 4, 40, sky=sky_with(4, low=1), overrides=fast, seed=14)
        dup = make_scenario("B1C", 4, 40, overrides=fast, seed=15)
        copy_channel(dup, 0, 3)
        c["duplicate_prn"] = dup
        c["b2a_6"] = make_scenario("B2A", 6, 700, overrides=dict(navSolPeriod=100), seed=16)
        idle = make_scenario("B1C", 6, 40, overrides=fast, seed=17)
        idle.status = "TT-TTT"
        idle.ephs[4] = dict(idle.ephs[4], flag=0)  # tracked, no ephemeris
        c["idle_and_no_eph"] = idle
    return _HOST_CASES


_HOST_CASES = {}


def track_results(scn, rng):
    """trackResults as the tracking step would leave them for a scenario: the three series, and prompt series that carry the
    scenario's navigation messages from each channel's subFrameStart on (B1C: Pilot_I_P with the secondary code, I_P with the
    frame; B2a: I_P with the three messages back to back)."""
    from bds_amd import synth

    import nav_cases as nc

    rows = []
    for c in range(scn.n_ch):
        first, prn = int(scn.subFrameStart[c]), int(scn.prns[c])
        r = SimpleNamespace(PRN=prn, status="T", absoluteSample=scn.absoluteSample[c], codeFreq=scn.codeFreq[c],
                            remCodePhase=scn.remCodePhase[c])
        if scn.signal == "B1C":
            starts = [i for i in (first, first + 1800) if i + 1799 <= scn.n]
            r.Pilot_I_P = nc.b1c_pilot(rng, scn.n, prn, starts)
            r.Pilot_Q_P = nc.noise_like(rng, scn.n)
            r.I_P = nc.noise_like(rng, scn.n)
            nc.place(r.I_P, first, synth.bcnav1_symbols(scn.msgs[c][0].copy(), fill=rng.integers(0, 2, 864)), rng, -1.0 if c % 2 else 1.0)
        else:
            r.I_P = nc.noise_like(rng, scn.n)
            for j, m in enumerate(scn.msgs[c]):
                nc.place(r.I_P, first + 3000 * j, synth.bcnav2_symbols(m[:264]), rng)
        rows.append(r)
    return rows
