"""Orbit-driven synthetic IF records (bds_synth_trajectory, bds_synth_traj; include/bds_mi355x.h, "driven by an orbit") for the
tests: the NumPy restatement of the per-sample arithmetic with the places at which it can silently go wrong as switches, the
record before the noise on a trajectory, the physical model solved directly in extended precision, and the scenarios.
Test infrastructure only; nothing here is loaded by the library.

  sample n, satellite     j = (n - first) >> seg_log2;  u = n - first - (j << seg_log2)
                          c = ((code[3] u + code[2]) u + code[1]) u + code[0];  k = floor(c / ncode);  cph = c - k ncode
                          period = period0 + k;  x = ((carr[3] u + carr[2]) u + carr[1]) u + carr[0]
                          th = 2 pi (x - trunc(x)) + phase;  from here on synth_cases.clean_record's lines
  truth                   rel solves rel = (t0 + n / fs) - delay(rel), delay = |R3(OmegaE_dot travel) pos - rx| / c - clk with
                          pvt_cases.satpos in np.longdouble; code = rel codeFreqBasis, carrier = IF n / fs - carrFreqBasis (delay - t0)
"""
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

import pvt_cases as pc
import synth_cases as sc

C_LIGHT = 299792458.0
NCODE = 10230


@dataclass(frozen=True)
class Model:
    horner: bool = True       # ((a3 u + a2) u + a1) u + a0; False: a0 + a1 u + a2 u^2 + a3 u^3, term by term
    trunc: bool = True        # x - trunc(x); False: x - floor(x)
    joint_next: bool = True   # sample first + (j + 1) 2^seg_log2 is the first of segment j + 1; False: the last of segment j
    period0: bool = True      # period = period0 + k; False: k alone


RIGHT = Model()
ALTERED = {"horner_order": Model(horner=False), "floor_for_trunc": Model(trunc=False), "joint_off_by_one": Model(joint_next=False),
           "period0_ignored": Model(period0=False)}


def _poly(a, u, model):
    if model.horner:
        return ((a[..., 3] * u + a[..., 2]) * u + a[..., 1]) * u + a[..., 0]
    return a[..., 0] + a[..., 1] * u + a[..., 2] * (u * u) + a[..., 3] * (u * u * u)


def sample_arith(segs, first, seg_log2, n, phase=0.0, model=RIGHT):
    """One satellite's row of segments (native.SYNTH_SEG_DTYPE [n_seg]) at samples n (int64 array) -> (j, u, cph, period, th),
    every float64 operation rounding once."""
    n = np.asarray(n, dtype=np.int64)
    m = n - np.int64(first)
    j = m >> np.int64(seg_log2)
    if not model.joint_next:
        j = np.where((m > 0) & ((m & ((1 << seg_log2) - 1)) == 0), j - 1, j)
    ui = m - (j << np.int64(seg_log2))
    u = ui.astype(np.float64)
    g = segs[j]
    c = _poly(g["code"], u, model)
    k = np.floor(c / float(NCODE))
    cph = c - k * float(NCODE)
    period = (g["period0"] if model.period0 else 0) + k.astype(np.int64)
    x = _poly(g["carr"], u, model)
    th = 2 * np.pi * (x - (np.trunc(x) if model.trunc else np.floor(x))) + phase
    return j, ui, cph, period, th


def fma(a, b, c):
    """fma(a, b, c) of float64 arrays, exactly: a b + c in integers (every double is an integer over a power of two), rounded once."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    out = np.empty(a.shape)
    flat = out.reshape(-1)
    for i, (x, y, z) in enumerate(zip(a.reshape(-1).tolist(), b.reshape(-1).tolist(), c.reshape(-1).tolist())):
        (nx, dx), (ny, dy), (nz, dz) = x.as_integer_ratio(), y.as_integer_ratio(), z.as_integer_ratio()
        flat[i] = (nx * ny * dz + nz * dx * dy) / (dx * dy * dz)  # int / int is correctly rounded
    return out


def sincos_strict(x):
    """csrc/bds_strict_math.h:sincos_strict line by line -> (sin, cos), bit for bit what the header gives."""
    x = np.asarray(x, dtype=np.float64)
    n = np.rint(x * 0.63661977236758134308)
    r = fma(-n, 1.57079632679489655800e+00, x)
    r = fma(-n, 6.12323399573676603587e-17, r)
    z = r * r
    ps = fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08)
    for coef in (2.75573137070700676789e-06, -1.98412698298579493134e-04, 8.33333333332248946124e-03, -1.66666666666666324348e-01):
        ps = fma(z, ps, coef)
    s0 = fma(z * r, ps, r)
    pc_ = fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09)
    for coef in (-2.75573143513906633035e-07, 2.48015872894767294178e-05, -1.38888888888741095749e-03, 4.16666666666666019037e-02):
        pc_ = fma(z, pc_, coef)
    hz = 0.5 * z
    w = 1.0 - hz
    c0 = w + (((1.0 - w) - hz) + z * (z * pc_))
    q = n.astype(np.int64)
    a, b = np.where(q & 1, c0, s0), np.where(q & 1, s0, c0)
    return np.where(q & 2, -a, a), np.where((q + 1) & 2, -b, b)


def clean_record(settings, sats, traj, first, n_samples, seed=3550, sigma=20.0, pilot61_secondary=False, symbol_table=None,
                 codegen=None, model=RIGHT):
    """The record before the noise on a trajectory (a synth.Trajectory, one row per entry of sats), complex128 -- the analytic
    signal; a real record is its real part, a conjugated record its conjugate -- in the device's own float64 operations, one
    rounding each and the satellites in list order, so that the device's format 0 equals the real part BIT FOR BIT:
    synth_cases.clean_record's lines with code phase, code period and carrier angle from sample_arith, sin / cos from the
    restated sincos_strict, and the product amp (s_I + j s_Q) e^{j th} written out as the kernel forms it."""
    from bds_amd import synth

    codegen = codegen or synth.default_codegen()
    fs = float(settings.samplingFreq)
    b1c = str(settings.signal).upper() == "B1C"
    sig = "B1C" if b1c else "B2A"
    prim = {s.prn: (np.asarray(codegen(sig, "data", s.prn), dtype=np.float64), np.asarray(codegen(sig, "pilot", s.prn), dtype=np.float64))
            for s in sats}
    n = np.arange(first, first + n_samples, dtype=np.int64)
    acc_i, acc_q = np.zeros(n_samples), np.zeros(n_samples)
    for k, s in enumerate(sats):
        amp = sigma * np.sqrt(4.0 * 10 ** (s.cn0_dbhz / 10) / fs)
        _, _, cph, pint, th = sample_arith(traj.segs[k], traj.first, traj.seg_log2, n, s.phase, model)
        ci = np.minimum(cph.astype(np.int64), NCODE - 1)
        if symbol_table is not None:
            tab = np.asarray(symbol_table)
            pidx = (pint + 1) % tab.shape[2]
            d_sym, p_sym = tab[k, 0][pidx].astype(np.float64), tab[k, 1][pidx].astype(np.float64)
        else:
            up, inv = np.unique(pint, return_inverse=True)
            d_sym, p_sym = sc.symbols(seed, up, s.prn, 0)[inv], sc.symbols(seed, up, s.prn, 1)[inv]
        cd, cp = prim[s.prn][0][ci], prim[s.prn][1][ci]
        if b1c:
            boc11 = 2.0 * (np.floor(cph * 2).astype(np.int64) & 1) - 1.0
            boc61 = np.where((np.floor(cph * 12).astype(np.int64) % 12) % 2 == 0, -1.0, 1.0)
            br = 0.5 * d_sym * cd * boc11 - np.sqrt(1.0 / 11.0) * cp * boc61 * (p_sym if pilot61_secondary else 1.0)
            bi = np.sqrt(29.0 / 44.0) * cp * boc11 * p_sym
        else:
            br, bi = p_sym * cp, -(d_sym * cd)
        ar, ai = amp * br, amp * bi
        sn, cs = sincos_strict(th)
        acc_i = acc_i + (ar * cs - ai * sn)
        acc_q = acc_q + (ar * sn + ai * cs)
    return acc_i + 1j * acc_q


def record_values(z, first, seed=3550, sigma=20.0, iq_sign=0):
    """The float64 values the quantiser sees, from the clean complex record z of samples first .. first + len(z)."""
    g_i, g_q = sc.noise_normals(seed, np.arange(first, first + z.size, dtype=np.int64))
    if not iq_sign:
        return z.real + sigma * g_i
    v = np.empty(2 * z.size)
    v[0::2] = z.real + sigma * g_i
    v[1::2] = (z.imag if iq_sign > 0 else -z.imag) + sigma * g_q
    return v


# ---- the tiny records of the bit-equality tests: 3 satellites, one PRN twice, samples 1000 .. 5119 of hand_made()'s trajectories --------
TINY_SEED, TINY_FIRST, TINY_N = 3550, 1000, 4120


def tiny_sats():
    from bds_amd import synth

    return [synth.Sat(19, 0.0, 0.0, 0.7, 47.0), synth.Sat(27, 0.0, 0.0, 2.9, 44.0), synth.Sat(19, 0.0, 0.0, 2.1, 41.0)]


# ---- hand-made trajectories for the bit-equality tests -----------------------------------------------------------------------------
def hand_made(settings, first=744, seg_log2=10, n_seg=6, roll_at=(2047, 2049, 3071)):
    """Three rows (the caller gives rows 0 and 2 one PRN) of `n_seg` segments of 2^seg_log2 samples from sample `first` on.  Every
    segment has its own cubic (continuity is the builder's business, not the device's), its own period0 -- negative in row 1 --
    and row k's code[0] is set so that the code period rolls over at sample first + roll_at[k]: one, two and three samples from a
    joint at sample first + 2048 / first + 3072 (seg_log2 10).  Row 2's carrier runs backwards (negative x)."""
    from bds_amd import native

    rng = np.random.default_rng(7)
    L = 1 << seg_log2
    rate = float(settings.codeFreqBasis) / float(settings.samplingFreq)
    segs = np.zeros((3, n_seg), dtype=native.SYNTH_SEG_DTYPE)
    for k in range(3):
        for j in range(n_seg):
            g = segs[k, j]
            g["period0"] = (-3 if k == 1 else 5 * k) + 2 * j
            r = rate * (1.0 + 3e-6 * (k - 1))
            g["code"] = [rng.uniform(100.0, 9000.0), r, rng.uniform(-1, 1) * 1e-12, rng.uniform(-1, 1) * 1e-17]
            f = (float(settings.IF) + 900.0 * (k + 1)) / float(settings.samplingFreq)
            g["carr"] = [rng.uniform(0.0, 1.0), -f if k == 2 else f, rng.uniform(-1, 1) * 1e-9, rng.uniform(-1, 1) * 1e-15]
        j, u = divmod(roll_at[k], L)  # code[0] so that c reaches ncode between offsets u - 1 and u of segment j
        g = segs[k, j]
        a = g["code"].copy()
        a[0] = 0.0
        g["code"][0] = NCODE - (float(_poly(a, np.float64(u), RIGHT)) - 0.4 * a[1])
    return SimpleNamespace(segs=segs, first=first, seg_log2=seg_log2, prns=None)


# ---- the physical model, solved directly ---------------------------------------------------------------------------------------------
def truth_phases(settings, eph, rx, tow, t0, n):
    """(code phase [chips since tow on the satellite's clock], carrier phase [cycles], delay [s]) of samples n in np.longdouble."""
    f = np.longdouble
    b1c = str(settings.signal).upper() == "B1C"
    fs, fc, fcarr, f_if = f(settings.samplingFreq), f(settings.codeFreqBasis), f(settings.carrFreqBasis), f(settings.IF)
    n = np.asarray(n, dtype=np.int64).astype(f)
    rxl = np.asarray(rx, dtype=f)
    a = f(t0) + n / fs
    d = np.full(n.shape, f(0.08))
    for _ in range(6):  # contracts by the range rate over c, ~3e-6 per step
        pos, clk = pc.satpos(f(tow) + (a - d), eph, b1c, dtype=np.longdouble)
        travel = np.sqrt(((pos - rxl) ** 2).sum(axis=-1)) / f(C_LIGHT)
        w = f(pc.OMEGAE_DOT) * travel
        rot = np.stack([np.cos(w) * pos[..., 0] + np.sin(w) * pos[..., 1], -np.sin(w) * pos[..., 0] + np.cos(w) * pos[..., 1], pos[..., 2]], axis=-1)
        d = np.sqrt(((rot - rxl) ** 2).sum(axis=-1)) / f(C_LIGHT) - clk
    return (a - d) * fc, f_if * (n / fs) - fcarr * (d - f(t0)), d


def sky_scenario(signal, seed=5):
    """Five satellites as pvt_cases.make_scenario makes them (default_sky: MEO and IGSO, e = 0 and 0.02): ephemerides, messages,
    receiver position and TOW."""
    scn = pc.make_scenario(signal, 5, 8, seed=seed)
    assert {e["SatType"] for e in scn.ephs} == {pc.MEO, pc.IGSO} and {e["e"] == 0 for e in scn.ephs} == {True, False}
    return scn


def phase_errors(settings, scn, traj, t0, n):
    """Worst |trajectory - truth| over the satellites at samples n, as metres of range: (code, carrier)."""
    f = np.longdouble
    worst_code = worst_carr = 0.0
    cph, period = traj.code_phase(n)
    x = traj.carrier_phase(n)
    for k, e in enumerate(scn.ephs):
        code, carr, _ = truth_phases(settings, e, scn.rx, scn.tow, t0, n)
        dc = (period[k].astype(f) * f(NCODE) + cph[k].astype(f)) - code
        dx = x[k].astype(f) - carr
        dx = dx - np.rint(dx)  # whole cycles are left out of a segment's polynomial
        worst_code = max(worst_code, float(np.abs(dc).max()) * C_LIGHT / float(settings.codeFreqBasis))
        worst_carr = max(worst_carr, float(np.abs(dx).max()) * C_LIGHT / float(settings.carrFreqBasis))
    return worst_code, worst_carr
