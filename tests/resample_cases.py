"""Inputs, references, tolerances and assertion functions for the kernels of the resampling conditioner (csrc/bds_resample.h: k_ff_extend,
k_ff_fir, k_ff_decimate, k_widen16), shared by tests/test_resample_cases.py (the CPU checks of the cases themselves, and NumPy models of the
kernels with one change each that the assertions must reject), tests/test_resample_stages_gpu.py (the kernels, through
tools/probe/resample_stages.hip) and tests/test_resample_block_gpu.py (the block the library makes of a record, through bds_acq_block).
The case-file format is tests/pfa_cases.py's.  NumPy only.

References
  extension    [2 x(1) - x(nfact+1:-1:2); x; 2 x(end) - x(end-1:-1:end-nfact)] on integers: exact.
  one pass     y(i) = sum_k b(k) u(i - k), u(m) = u(0) for m < 0 (filter(b, 1, u, zi u(1)) with the steady-state zi of an FIR filter),
               accumulated in numpy.longdouble (64-bit significand here; double-double where it has fewer bits).  The reverse pass is
               flip(pass(flip(u))).  A(i) = sum_k |b(k)| |u(i - k)| in float64.
  decimation   index = ceil((0 : sig_len - 1) / fs' * fs), index(1) = 1, in float64 and in the operation order of oracle/acquisition.py:82.
  filtfilt     the three composed: extend, forward pass, reverse pass, decimate.

Tolerances are derived, not measured.  The kernel accumulates one output in a chain of T = n_taps fused multiply-adds, which errs by at most
gamma_T A(i), gamma_T = T u / (1 - T u), u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1; an FMA rounds
once per term).  T u < 4e-13 here, so gamma_T < T u (1 + 1e-12), and
  tol1(i) = 1.01 T u A(i)
leaves 1 % for the rounding of A itself (relative error < (T + 1) u) and of the long-double reference (T 2^-64 A(i) = T u A(i) / 2048).
The second pass filters y1' = y1 + e1, |e1| <= tol1, so it errs by at most gamma_T (|b| * |y1'|) + (|b| * tol1), and with
|y1'| <= |y1| + tol1 (the cross term gamma_T (|b| * tol1) is below 4e-13 of the second term, inside the 1 %):
  tol2(j) = 1.01 T u (|b| * |y1|)(j) + (|b| * tol1)(j),
* the same clamped-edge sum, run in the direction of the second pass.  No absolute floor, no fitted constant: where A is 0 (every
product of the chain is 0) the output must be the reference exactly.
"""
import functools
import os
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from pfa_cases import read_arrays, write_arrays  # noqa: F401

MAGIC = 0x52534D5053544147  # "RSMPSTAG"
GUARD = 64                   # doubles behind every output of the driver
FILL = 0x7FF8A5C31E870BD5    # the NaN every output and every guard is prefilled with
U = 2.0 ** -53
LONGDOUBLE_BITS = int(np.finfo(np.longdouble).nmant)
_WORKERS = max(1, min(8, os.cpu_count() or 1))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))


# ---- references ------------------------------------------------------------------------------------------------------------------
def extend_ref(x, nfact):
    """The literal MATLAB expression on integers (int64), along axis 0."""
    x = np.asarray(x).astype(np.int64)
    n = x.shape[0]
    assert n > nfact >= 0
    head = 2 * x[0] - x[nfact:0:-1]                                   # x(nfact+1:-1:2)
    tail = 2 * x[n - 1] - x[[n - 2 - j for j in range(nfact)]]        # x(end-1:-1:end-nfact)
    return np.concatenate([head, x, tail])


def _padded(u, n_taps, dtype):
    u = np.asarray(u, dtype=dtype)
    return np.concatenate([np.full(n_taps - 1, u[0], dtype=dtype), u])


def _two_sum(a, b):
    s = a + b
    t = s - a
    return s, (a - (s - t)) + (b - t)


def _two_prod(a, b):
    p = a * b
    ah, bh = a * 134217729.0, b * 134217729.0  # Veltkamp split, 2^27 + 1
    ah, bh = ah - (ah - a), bh - (bh - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def pass_ref_dd(u, b):
    """The pass in double-double (about 106 bits), for a numpy.longdouble that is no wider than float64.  Returns (hi, lo)."""
    b = np.asarray(b, dtype=np.float64)
    t, n = len(b), len(u)
    up = _padded(u, t, np.float64)
    hi, lo = np.zeros(n), np.zeros(n)
    for k in range(t):
        p, e = _two_prod(np.full(n, b[k]), up[t - 1 - k:t - 1 - k + n])
        hi, s = _two_sum(hi, p)
        lo += s + e
        hi, lo = _two_sum(hi, lo)
    return hi, lo


def pass_ref(u, b):
    """y(i) = sum_k b(k) u(i - k), u(m) = u(0) for m < 0, as numpy.longdouble [len]; u float64 or longdouble."""
    t, n = len(b), len(u)
    if LONGDOUBLE_BITS < 63:
        if np.asarray(u).dtype == np.longdouble:
            raise NotImplementedError("a second pass needs numpy.longdouble wider than float64")
        hi, lo = pass_ref_dd(u, b)
        return hi.astype(np.longdouble) + lo
    w = sliding_window_view(_padded(u, t, np.longdouble), t)  # w[i, j] = u(i - (t - 1) + j)
    br = np.asarray(b, dtype=np.longdouble)[::-1].copy()
    if n * t < 1 << 24:
        return w @ br
    cuts = np.linspace(0, n, 4 * _WORKERS + 1).astype(np.int64)
    with ThreadPoolExecutor(_WORKERS) as ex:
        return np.concatenate(list(ex.map(lambda i: w[cuts[i]:cuts[i + 1]] @ br, range(len(cuts) - 1))))


def reverse_ref(u, b):
    return pass_ref(np.asarray(u)[::-1], b)[::-1]


def pass_abs(u, b):
    """A(i) = sum_k |b(k)| |u(i - k)| in float64, same clamped edge."""
    b = np.abs(np.asarray(b, dtype=np.float64))
    return np.convolve(np.abs(_padded(u, len(b), np.float64)), b, mode="valid")


def tol1_of(u, b):
    return 1.01 * len(b) * U * pass_abs(u, b)


def tol2_of(y1, t1, b):
    """The tolerance behind the REVERSE pass over y1 (the reference's first-pass output) that carries the tolerance t1."""
    y1 = np.abs(np.asarray(y1)).astype(np.float64)
    return (1.01 * len(b) * U * pass_abs(y1[::-1], b) + pass_abs(t1[::-1], b))[::-1]


def decimate_index(sig_len, new_fs, old_fs):
    """index (1-based) of B2a/acquisition.m:109-110, in the float64 operation order of oracle/acquisition.py:82."""
    idx = np.ceil(np.arange(sig_len, dtype=np.float64) / new_fs * old_fs).astype(np.int64)
    idx[0] = 1
    return idx


def sig_len_of(n_in, new_fs, old_fs):
    return int(np.floor((n_in - 1) / old_fs * new_fs))  # oracle/acquisition.py:81


FiltRef = namedtuple("FiltRef", "ref tol idx")


def filtfilt_ref(x, b, new_fs, old_fs):
    """x: integers [n] -> the conditioned block (longdouble [sig_len]), tol2 per sample, and the 1-based indices selected."""
    nfact = 3 * (len(b) - 1)
    e = extend_ref(x, nfact).astype(np.float64)
    y1 = pass_ref(e, b)
    t1 = tol1_of(e, b)
    y2 = reverse_ref(y1, b)
    t2 = tol2_of(y1, t1, b)
    idx = decimate_index(sig_len_of(len(x), new_fs, old_fs), new_fs, old_fs)
    out = FiltRef(y2[nfact + idx - 1], t2[nfact + idx - 1], idx)
    for a in out:
        a.setflags(write=False)
    return out


def worst_ratio(got, ref, tol):
    """max |got - ref| / tol; where tol is 0 the output must be the reference exactly (then the ratio is 0).  Raises above 1."""
    got, ref, tol = np.asarray(got), np.asarray(ref), np.asarray(tol)
    assert got.shape == ref.shape == tol.shape, (got.shape, ref.shape, tol.shape)
    assert np.all(np.isfinite(got)), "an output is not finite (never written?)"
    err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
    zero = tol == 0
    assert not np.any(err[zero] != 0), "an output whose every product is 0 differs from the reference"
    r = float(np.max(err[~zero] / tol[~zero])) if np.any(~zero) else 0.0
    assert r <= 1.0, f"error / tolerance = {r:.3e} at {int(np.argmax(np.where(zero, 0, err / np.where(zero, 1, tol))))}"
    return r


# ---- the band-pass sampling plan (csrc/bds_resample.h resample_plan; oracle/acquisition.py:59-85) -----------------------------------
def plan_rates(fs, IF, bw):
    fu, fl = IF + bw / 2, IF - bw / 2
    n = max(1, int(np.floor(fu / bw)))
    lower = 2 * fu / n
    upper = 2 * fl / (n - 1) if n > 1 else lower
    return float(np.ceil((lower + upper) / 2))


B1C_53_NEW_FS = plan_rates(53e6, 14.58e6, 9e6)  # B1C/initSettings.m's rate and IF


# ---- k_ff_extend -----------------------------------------------------------------------------------------------------------------
ExtendCase = namedtuple("ExtendCase", "name nch width nfact x")  # x: int8 / int16 [n, nch]
EXTEND_SHAPES = ((2100, 2101), (2100, 2102), (2100, 4200), (2100, 5000), (6, 7))
EXTEND_BIG = 530000  # > 2048 x 256: a second trip of the grid-stride loop


def _extend_input(seed, n, nch, width):
    lo, hi = (-128, 127) if width == 8 else (-32768, 32767)
    x = np.stack([np.random.default_rng([seed, c]).integers(lo, hi + 1, n) for c in range(nch)], axis=1)  # I and Q: two streams
    x[0], x[n - 1] = [hi, lo][:nch], [lo, hi][:nch]  # 2 x - x' reaches three times the range
    x[1, 0], x[n - 2, 0] = lo, hi                    # ... at the first reflected element of both ends
    return x.astype(np.int8 if width == 8 else np.int16)


@functools.lru_cache(maxsize=None)
def extend_cases():
    cases = [ExtendCase(f"<{nch},int{width}> nfact {nfact} n {n}", nch, width, nfact, _extend_input(7 * n + nch + width, n, nch, width))
             for nch in (1, 2) for width in (8, 16) for nfact, n in EXTEND_SHAPES]
    cases += [ExtendCase(f"<{nch},int{width}> nfact 2100 n {EXTEND_BIG}", nch, width, 2100, _extend_input(99 + nch, EXTEND_BIG, nch, width))
              for nch, width in ((1, 8), (2, 16))]
    return tuple(cases)


def assert_extend(case, got):
    """got: float64 [(n + 2 nfact), nch]: bit for bit the extension."""
    ref = extend_ref(case.x, case.nfact).astype(np.float64)
    assert np.abs(ref).max() > (2.9 * 127 if case.width == 8 else 2.9 * 32767)
    bad = np.argwhere(bits(got).reshape(ref.shape) != bits(ref))
    assert not len(bad), (case.name, "first differing (sample, channel)", bad[0].tolist(), len(bad))
    return 0.0


# ---- k_widen16 -------------------------------------------------------------------------------------------------------------------
WIDEN_N = (1, 255, 257, 600000)


@functools.lru_cache(maxsize=None)
def widen_cases():
    out = []
    for n in WIDEN_N:
        x = np.random.default_rng(n).integers(-32768, 32768, n).astype(np.int16)
        x[[0, n // 3, n // 2, n - 1][:min(n, 4)]] = [-32768, 32767, -32767, 32767][:min(n, 4)]
        if n == 1:
            x[0] = -32768
        out.append(x)
    return tuple(out)


def assert_widen(x, got):
    assert same_bits(got, x.astype(np.float64)), ("k_widen16", len(x))
    return 0.0


# ---- k_ff_decimate ---------------------------------------------------------------------------------------------------------------
DecCase = namedtuple("DecCase", "name nch nfact sig_len new_fs old_fs")
# (old, new, sig_len, the k at which one of the three neighbouring evaluation orders first parts from the reference: tests/test_resample_cases.py)
DEC_PAIRS = ((40e6, 29e6, 4000, (29, 87, 145)),
             (99.375e6, 19.62e6, 25000, (11772, 22236)),
             (99.375e6, 48.06e6, 60000, (16020, 54468)),
             (53e6, B1C_53_NEW_FS, 25000, ()))
DEC_BIG = 530000


def decimate_cases():
    cases = [DecCase(f"{old / 1e6:g}->{new / 1e6:g} nch {nch} nfact {nfact}", nch, nfact, n, new, old)
             for old, new, n, _ in DEC_PAIRS for nch in (1, 2) for nfact in (0, 2100)]
    cases.append(DecCase(f"99.375->48.06 nch 1 nfact 2100 sig_len {DEC_BIG}", 1, 2100, DEC_BIG, 48.06e6, 99.375e6))
    return tuple(cases)


def other_orders(sig_len, new_fs, old_fs):
    """The three neighbouring evaluation orders of the index (1-based, k = 0 -> 1 as the reference)."""
    k = np.arange(sig_len, dtype=np.float64)
    out = {}
    for name, v in (("k*(old/new)", k * (old_fs / new_fs)), ("k*old/new", k * old_fs / new_fs), ("k*(1/new)*old", k * (1.0 / new_fs) * old_fs)):
        idx = np.ceil(v).astype(np.int64)
        idx[0] = 1
        out[name] = idx
    return out


def decimate_input(case):
    """z[i] = i (channel 1: i + 0.5), long enough for the reference's largest index and two more (so that an evaluation order
    that lands one sample later still reads inside the buffer)."""
    zlen = case.nfact + int(decimate_index(case.sig_len, case.new_fs, case.old_fs).max()) + 2
    z = np.arange(zlen, dtype=np.float64)
    return z[:, None] + np.array([0.0, 0.5][:case.nch])[None, :]


def assert_decimate(case, got):
    """got float64 [sig_len, nch]: the output names the index it was read from."""
    ref = (case.nfact + decimate_index(case.sig_len, case.new_fs, case.old_fs) - 1).astype(np.float64)[:, None] + np.array([0.0, 0.5][:case.nch])[None, :]
    bad = np.argwhere(bits(got).reshape(ref.shape) != bits(ref))
    assert not len(bad), (case.name, "first differing (k, channel)", bad[0].tolist(), len(bad))
    return 0.0


# ---- k_ff_fir --------------------------------------------------------------------------------------------------------------------
FIR_TAPS = (1, 2, 255, 256, 257, 701)  # around the 256-thread staging loop of s_b
FIR_MIN_LEN = 6301                     # the shortest extended block the library makes: 2101 + 2 x 2100
FIR_BIG = 534200                       # 530 000 + 2 x 2100: a second trip of the grid-stride loop
SIGNALS = ("normal", "normal2", "constant", "impulse0", "impulse_mid", "impulse_last")
PAIRS = ((0, 1), (2, 3), (4, 5))       # the signals an NCH = 2 run interleaves
FirGroup = namedtuple("FirGroup", "name b signals")  # signals float64 [6, len]


def fir_lengths(n_taps):
    return sorted({v for v in (1, n_taps - 1, n_taps, n_taps + 1, 3 * n_taps, FIR_MIN_LEN) if v >= 1})


def taps_of(kind, n_taps):
    """'fir1': a symmetric band-pass design as fir1 makes (B2a's band edges; lengths 1 and 2 have no window design: [1], [1/2, 1/2]);
    'asym': random taps, no symmetry."""
    if kind == "asym":
        return np.random.default_rng(1000 + n_taps).standard_normal(n_taps) / np.sqrt(n_taps)
    if n_taps < 3:
        return np.full(n_taps, 1.0 / n_taps)
    m = np.arange(n_taps) - 0.5 * (n_taps - 1)
    wp1, wp2 = 0.0648805, 0.4845195
    h = (wp2 * np.sinc(wp2 * m) - wp1 * np.sinc(wp1 * m)) * (0.54 - 0.46 * np.cos(2 * np.pi * np.arange(n_taps) / (n_taps - 1)))
    h = 0.5 * (h + h[::-1])  # symmetric to the bit
    return h / abs(np.sum(h * np.cos(np.pi * m * 0.5 * (wp1 + wp2))))


def impulse_positions(n):
    return 0, n // 2, n - 1


@functools.lru_cache(maxsize=None)
def fir_group(kind, n_taps, n):
    rng = np.random.default_rng([n_taps, n, kind == "asym"])
    s = np.zeros((6, n))
    s[0], s[1] = 100.0 * rng.standard_normal(n), 100.0 * rng.standard_normal(n)
    s[2] = 73.25
    for i, p in enumerate(impulse_positions(n)):
        s[3 + i, p] = 1.0
    s.setflags(write=False)
    b = taps_of(kind, n_taps)
    b.setflags(write=False)
    return FirGroup(f"{kind} taps {n_taps} len {n}", b, s)


def fir_groups(n_taps):
    return [fir_group(kind, n_taps, n) for kind in ("fir1", "asym") for n in fir_lengths(n_taps)]


def fir_jobs(group):
    """[(key, reverse, u float64 [len, nch])]: per signal the forward run, the reverse run and the forward run of the flipped signal
    (NCH = 1); per pair the forward and the reverse run (NCH = 2)."""
    s = group.signals
    jobs = []
    for i in range(len(s)):
        jobs += [(("f", i), 0, s[i][:, None]), (("r", i), 1, s[i][:, None]), (("ff", i), 0, s[i][::-1][:, None])]
    for p, (i, j) in enumerate(PAIRS):
        u = np.stack([s[i], s[j]], axis=1)
        jobs += [(("f2", p), 0, u), (("r2", p), 1, u)]
    return jobs


def impulse_response(b, n, p):
    """What a forward pass makes of a unit impulse at p, bit for bit: the taps, or -- p = 0, where the clamp repeats the impulse in
    front of the block -- the running sum of the taps from the oldest sample to the newest (an FMA by 1 is an addition)."""
    y = np.zeros(n)
    if p == 0:
        run = np.cumsum(b[::-1])[::-1]  # run[i] = ((b[T-1] + b[T-2]) + ...) + b[i]
        m = min(n, len(b))
        y[:m] = run[:m]
    else:
        m = min(n - p, len(b))
        y[p:p + m] = b[:m]
    return y


def assert_fir_group(group, res):
    """res: key -> float64 [len, nch] for every job of fir_jobs(group).  Every output within tol1 of the long-double reference; the
    impulses bit for bit; reverse = flip(forward(flip)) and NCH = 2 = NCH = 1 per channel as bits.  Returns the largest error / tol1."""
    b, s = group.b, group.signals
    n = s.shape[1]
    worst = 0.0
    for i in range(len(s)):
        f, r, ff = (res[(k, i)].reshape(n) for k in ("f", "r", "ff"))
        what = (group.name, SIGNALS[i])
        worst = max(worst, worst_ratio(f, pass_ref(s[i], b), tol1_of(s[i], b)))
        flipped = s[i][::-1]
        yf, tf = pass_ref(flipped, b), tol1_of(flipped, b)
        worst = max(worst, worst_ratio(ff, yf, tf), worst_ratio(r, yf[::-1], tf[::-1]))
        assert same_bits(r, ff[::-1]), what + ("the reverse pass is not flip(forward(flip))",)
        if i >= 3:
            p = impulse_positions(n)[i - 3]
            assert same_bits(f, impulse_response(b, n, p)), what + ("forward",)
            assert same_bits(r, impulse_response(b, n, n - 1 - p)[::-1]), what + ("reverse",)
    for p, (i, j) in enumerate(PAIRS):
        for k2, k1 in (("f2", "f"), ("r2", "r")):
            got = res[(k2, p)].reshape(n, 2)
            assert same_bits(got[:, 0], res[(k1, i)].reshape(n)) and same_bits(got[:, 1], res[(k1, j)].reshape(n)), \
                (group.name, k2, "a channel of the NCH = 2 run is not the NCH = 1 run on it")
    return worst


@functools.lru_cache(maxsize=None)
def fir_big():
    """One signal of FIR_BIG samples, 701 asymmetric taps, with its references: (b, u, forward ref, its tol, ref and tol of flip(u))."""
    b = taps_of("asym", 701)
    u = 100.0 * np.random.default_rng(534200).standard_normal(FIR_BIG)
    out = (b, u, pass_ref(u, b), tol1_of(u, b), pass_ref(u[::-1], b), tol1_of(u[::-1], b))
    for a in out:
        a.setflags(write=False)
    return out


def assert_fir_big(f, r, ff):
    b, u, yf, tf, yr, tr = fir_big()
    worst = max(worst_ratio(f, yf, tf), worst_ratio(ff, yr, tr), worst_ratio(r, yr[::-1], tr[::-1]))
    assert same_bits(r, ff[::-1]), "the reverse pass is not flip(forward(flip))"
    return worst


# ---- NumPy models of the kernels, with one change each on request -----------------------------------------------------------------
def model_extend(x, nfact, mutant=None):
    x = np.asarray(x).astype(np.float64)
    n = x.shape[0]
    head = -x[nfact:0:-1] if mutant == "head reflection without 2 x(0)" else 2.0 * x[0] - x[nfact:0:-1]
    first = n - 1 if mutant == "tail reflection shifted by one" else n - 2
    tail = 2.0 * x[n - 1] - x[[max(first - j, 0) for j in range(nfact)]]
    e = np.concatenate([head, x, tail])
    return e[:, ::-1] if mutant == "I and Q exchanged" else e


def model_fir(u, b, reverse, mutant=None):
    """u float64 [len, nch]: the kernel's loop in plain sequential float64 (a multiplication and an addition per tap: no FMA), taps from
    the oldest sample to the newest."""
    u = np.asarray(u, dtype=np.float64)
    n, t = u.shape[0], len(b)
    if mutant == "forward and reverse pass exchanged":
        reverse = not reverse
    if mutant == "taps in the other direction":
        b = b[::-1]
    v = u[::-1] if reverse else u
    first = v[min(1, n - 1)] if mutant == "clamp to u(1)" else v[0] * (0.0 if mutant == "steady-state start replaced by zeros" else 1.0)
    vp = np.concatenate([np.repeat(first[None, :], t - 1, axis=0), v])
    acc = np.zeros_like(v)
    for k in range(t - 1, -1, -1):
        acc = acc + b[k] * vp[t - 1 - k:t - 1 - k + n]
    if mutant == "I and Q exchanged":
        acc = acc[:, ::-1]
    return np.ascontiguousarray(acc[::-1] if reverse else acc)


def model_decimate(z, nfact, sig_len, new_fs, old_fs, mutant=None):
    k = np.arange(sig_len, dtype=np.float64)
    if mutant in ("k*(old/new)", "k*old/new", "k*(1/new)*old"):
        idx = other_orders(sig_len, new_fs, old_fs)[mutant]
    else:
        idx = (np.floor if mutant == "floor for ceil" else np.ceil)(k / new_fs * old_fs).astype(np.int64)
        if mutant != "k == 0 rule dropped":
            idx[0] = 1
    out = z[np.maximum(idx - 1 + nfact, 0)]
    return out[:, ::-1] if mutant == "I and Q exchanged" else out


def model_group(group, mutant=None):
    return {key: model_fir(u, group.b, rev, mutant) for key, rev, u in fir_jobs(group)}


# ---- case files of tools/probe/resample_stages.hip --------------------------------------------------------------------------------
def job_extend(case):
    return [np.array([1, case.nch, case.width, case.x.shape[0], case.nfact], dtype=np.int64), case.x]


def job_fir(u, b, reverse):
    return [np.array([2, u.shape[1], u.shape[0], len(b), int(reverse)], dtype=np.int64), np.ascontiguousarray(u, dtype=np.float64),
            np.ascontiguousarray(b, dtype=np.float64)]


def job_decimate(case):
    z = decimate_input(case)
    return [np.array([3, case.nch, case.nfact, case.sig_len, z.shape[0]], dtype=np.int64), np.array([case.new_fs, case.old_fs]), z]


def job_widen(x):
    return [np.array([4, len(x)], dtype=np.int64), x]


def case_file(jobs):
    return [np.array([MAGIC, len(jobs)], dtype=np.int64)] + [a for j in jobs for a in j]


def split_output(raw, shape):
    """One result array of the driver -> the output in `shape`, after checking that every element was written and the guard behind it
    was not."""
    w = np.asarray(raw).view(np.uint64)
    n = int(np.prod(shape))
    assert w.size == n + GUARD, (w.size, n)
    assert np.all(w[n:] == np.uint64(FILL)), "the guard behind an output was written"
    assert not np.any(w[:n] == np.uint64(FILL)), "an output element was never written"
    return w[:n].view(np.float64).reshape(shape)


# ---- the blocks of tests/test_resample_block_gpu.py --------------------------------------------------------------------------------
def shortest_input(n_needed, new_fs, old_fs, nfact=2100):
    """The smallest n_in whose resampled block has at least n_needed samples (and that filtfilt accepts)."""
    n = max(nfact + 1, int(np.floor(n_needed * old_fs / new_fs)) - 2)
    while sig_len_of(n, new_fs, old_fs) < n_needed:
        n += 1
    return n
