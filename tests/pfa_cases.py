"""Inputs and float64 references for the stages of the N-point search pair (csrc/bds_acq_pfa.h), shared by tests/test_pfa_cases.py
(the CPU checks of the cases themselves) and tests/test_pfa_stages_gpu.py (the kernels, through tools/probe/pfa_stages.hip).

NumPy only.  Every reference is numpy.fft in float64 over the Good-Thomas index maps of the header:
  spectrum index k <-> (k1, k2, k3) = (k mod 53, k mod 12, k mod 3125),   lag_of(t1, t2, t3) = (t1 N/53 + t2 N/12 + t3 N/3125) mod N,
  bw_piece(mp, k2, t3) for the tiled inter-pass buffer;
direct sums at sampled outputs (direct_*) keep the FFT-based references honest.

Column-pass inputs are built in the LAG domain, so that peaks can be planted at chosen (t1, t2, t3): y[2][53][12][3125] = a noise
floor + planted values, Bw = forward 53 x 12 transform of y / 636 rounded to fp16, and the reference is computed from the ROUNDED
buffer: that isolates the pass from the storage error.
"""
import functools
from collections import namedtuple

import numpy as np

K1, K2, K3 = 53, 12, 3125
NP = K1 * K2 * K3  # 1 987 500
MP = 27
TILE = 16
TILES = (K3 + TILE - 1) // TILE  # 196
CELL_ELEMS = TILES * MP * K2 * TILE * 4
W0 = float(np.float32(0.52440442))  # the magnitude weights and the sieve tolerance of a B1C run, as the kernel holds them (fp32)
W1 = float(np.float32(0.85146932))
WSUM2 = W0 * W0 + W1 * W1
KEEP = float(np.float32(0.996))
# Ambiguity band: twice the fp32 budget of the sieve arithmetic (1e-5 of the maximum, kDelta / 2 at fp32 storage).  A lag whose
# reference value is within +-BAND of a threshold is asserted neither way -- and every case has NO such lag (tests/test_pfa_cases.py).
BAND = 2e-5
WAVE_ITEMS_PER_CELL = 195 * 4 + 2  # waves with t0 = 16 tile + 4 wave < 3125

MAGIC = 0x5046415354414745
GUARD_WORD = 0xA5C31E87
GUARD_EXTRA = 4096


# ---- index maps ----------------------------------------------------------------------------------------------------------------
def lag_of(t1, t2, t3):
    t1, t2, t3 = (np.asarray(v, dtype=np.int64) for v in (t1, t2, t3))
    return (t1 * (NP // K1) + t2 * (NP // K2) + t3 * (NP // K3)) % NP


def bw_piece(mp, k2, t3):
    """Element index (fp16 complex, 4 bytes) of the 4-element piece of (mp, k2, t3) in its cell."""
    return ((t3 // TILE * MP + mp) * K2 + k2) * (TILE * 4) + (t3 % TILE) * 4


@functools.lru_cache(maxsize=None)
def crt_index():
    """k_of[k1, k2, k3] = the natural index k with (k mod 53, k mod 12, k mod 3125) = (k1, k2, k3)."""
    k = np.arange(NP, dtype=np.int64)
    k_of = np.empty((K1, K2, K3), dtype=np.int64)
    k_of[k % K1, k % K2, k % K3] = k
    k_of.setflags(write=False)
    return k_of


@functools.lru_cache(maxsize=None)
def lag_grid():
    """(lag[t1, t2, t3], its inverse: grid position (flat index into [53][12][3125]) of every lag)."""
    lag = lag_of(np.arange(K1)[:, None, None], np.arange(K2)[None, :, None], np.arange(K3)[None, None, :])
    inv = np.empty(NP, dtype=np.int64)
    inv[lag.ravel()] = np.arange(NP, dtype=np.int64)
    lag.setflags(write=False)
    inv.setflags(write=False)
    return lag, inv


# ---- fp16 storage ---------------------------------------------------------------------------------------------------------------
def pack_h2(z):
    """complex -> uint32 (re in the low half, im in the high half), each part rounded to fp16 (nearest even)."""
    z = np.asarray(z)
    re = z.real.astype(np.float16).view(np.uint16).astype(np.uint32)
    im = z.imag.astype(np.float16).view(np.uint16).astype(np.uint32)
    return re | (im << np.uint32(16))


def unpack_h2(u):
    u = np.ascontiguousarray(u, dtype=np.uint32)
    re = (u & np.uint32(0xFFFF)).astype(np.uint16).view(np.float16).astype(np.float64)
    im = (u >> np.uint32(16)).astype(np.uint16).view(np.float16).astype(np.float64)
    return re + 1j * im


def round_h2(z):
    return unpack_h2(pack_h2(z))


def bw_pack(z):
    """z[2][53][12][3125] (fp16-exact values) -> a cell of the inter-pass buffer.  The pad row k1 = 53 is zero, as the row pass
    leaves it; the 11 pad lags of the last tile hold 0xffffffff (two fp16 NaNs), as the library's prefill leaves them: no kernel may
    read them."""
    full = np.full((2, 2 * MP, K2, TILES * TILE), 0xFFFFFFFF, dtype=np.uint32)
    full[:, :K1, :, :K3] = pack_h2(z)
    full[:, K1, :, :K3] = 0
    # (c, mp, row, k2, tile, lag) -> [tile][mp][k2][lag][c][row]
    return np.ascontiguousarray(full.reshape(2, MP, 2, K2, TILES, TILE).transpose(4, 1, 3, 5, 0, 2)).reshape(-1)


def bw_unpack_words(cell):
    """A cell of the inter-pass buffer -> its words as [2][54][12][3136] (pad row and pad lags included)."""
    w = np.asarray(cell, dtype=np.uint32).reshape(TILES, MP, K2, TILE, 2, 2)
    return np.ascontiguousarray(w.transpose(4, 1, 5, 2, 0, 3)).reshape(2, 2 * MP, K2, TILES * TILE)


# ---- case files of tools/probe/pfa_stages.hip ------------------------------------------------------------------------------------
def write_arrays(path, arrays):
    with open(path, "wb") as f:
        f.write(np.int64(len(arrays)).tobytes())
        for a in arrays:
            b = np.ascontiguousarray(a).tobytes()
            f.write(np.int64(len(b)).tobytes())
            f.write(b)
            f.write(b"\0" * (-len(b) % 8))


def read_arrays(path):
    with open(path, "rb") as f:
        buf = f.read()
    n = int(np.frombuffer(buf, np.int64, 1, 0)[0])
    out, off = [], 8
    for _ in range(n):
        ln = int(np.frombuffer(buf, np.int64, 1, off)[0])
        out.append(np.frombuffer(buf, np.uint8, ln, off + 8))
        off += 8 + (ln + 7) // 8 * 8
    return out


Launch = namedtuple("Launch", "ncells cell0 lb_div qchunk grid extra_cap stats keep")


def launch_table(launches):
    return np.array([[l.ncells, l.cell0, l.lb_div, l.qchunk, l.grid, l.extra_cap, int(l.stats), l.keep, W0, W1] for l in launches], dtype=np.float64).reshape(-1, 10)


def items_of(ncells, qchunk):
    return (TILES + qchunk - 1) // qchunk * qchunk * ncells


def host_grid(ncells, qchunk):
    """The column grid csrc/bds_acq.hip launches for a cell list of this size."""
    items = items_of(ncells, qchunk)
    return min(items, max(512, min(8192, items // 24)))


ColsResult = namedtuple("ColsResult", "cellmax_v cellmax_lag lb count stats head_guard entries tail_guard")
EXTRA_DT = np.dtype([("v", "<f4"), ("lag", "<i4"), ("cell", "<i4")])


def parse_cols(arrays):
    """The five result arrays of one column launch."""
    cm, lb, count, stats, ex = arrays
    cm = cm.view(np.uint64)
    ex = ex.view(EXTRA_DT)
    val = (cm >> np.uint64(32)).astype(np.uint32).view(np.float32)
    lag = (~cm & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return ColsResult(val, lag, lb.view(np.float32), int(count.view(np.int32)[0]), stats.view(np.uint64).astype(np.int64), ex[:GUARD_EXTRA],
                      ex[GUARD_EXTRA:len(ex) - GUARD_EXTRA], ex[len(ex) - GUARD_EXTRA:])


def guard_intact(words):
    return bool(np.all(np.asarray(words).view(np.uint32) == np.uint32(GUARD_WORD)))


# ---- forward transforms ---------------------------------------------------------------------------------------------------------
FWD_SCALE = 1.0 / 65536.0


@functools.lru_cache(maxsize=None)
def forward_input():
    """Two integer-valued signals (exact in fp32, so the float64 reference sees what the kernel sees)."""
    rng = np.random.default_rng(11)
    x = np.round(20.0 * rng.standard_normal((2, NP))) + 1j * np.round(3.0 * rng.standard_normal((2, NP)))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def forward_reference():
    """fft(x) * scale in the CRT layout [batch][53][12][3125] (not conjugated)."""
    X = np.fft.fft(forward_input(), axis=-1) * FWD_SCALE
    ref = X[:, crt_index()]
    ref.setflags(write=False)
    return ref


def forward_case(nb, doubled, conj, stride):
    x = forward_input()[:nb]
    xs = np.empty((nb, NP, 2), dtype=np.float32)
    xs[..., 0], xs[..., 1] = x.real, x.imag
    return [np.array([MAGIC, 1, nb, doubled, conj, stride], dtype=np.int64), np.array([FWD_SCALE]), xs]


@functools.lru_cache(maxsize=None)
def _unit_table():
    return np.exp(2j * np.pi * np.arange(NP) / NP)


def direct_npoint(x, k, sign):
    """sum_n x[n] exp(sign 2 pi j n k / N) of a natural-order x, one output k."""
    n = np.arange(NP, dtype=np.int64)
    w = _unit_table()[(n * int(k)) % NP]
    return np.sum(x * (w if sign > 0 else np.conj(w)))


# ---- row pass -------------------------------------------------------------------------------------------------------------------
NSLOTS = 2
RowsRun = namedtuple("RowsRun", "name bins slots gc shift")
# Rotations s = bin * shift in {0, 1, 11, 12, 52, 53, 200} and 400 (shift 2, bin 200): 0, the first step, around the periods of the
# 12- and the 53-point dimension and the last bin of the search band.  Five cells in chunks of two: a short last chunk, and the PRN
# slot changes from chunk to chunk (cs[c0] serves the whole chunk).  Then one cell per chunk.
ROWS_RUNS = (
    RowsRun("gc2", (0, 1, 11, 12, 52), (0, 0, 1, 1, 0), 2, 1),
    RowsRun("gc1", (53, 200, 12), (1, 0, 1), 1, 1),
    RowsRun("shift2", (200, 0, 6), (0, 0, 1), 2, 2),
)
ROWS_GUARD = TILE * MP * K2 * 4  # elements in front of and behind the destination: one tile


@functools.lru_cache(maxsize=None)
def rows_spectra():
    """(Xnat[N], Cnat[slot][component][N]): fp16-exact spectra in natural order."""
    rng = np.random.default_rng(7)
    X = round_h2(8.0 * (rng.standard_normal(NP) + 1j * rng.standard_normal(NP)))
    C = round_h2(0.125 * (rng.standard_normal((NSLOTS, 2, NP)) + 1j * rng.standard_normal((NSLOTS, 2, NP))))
    X.setflags(write=False)
    C.setflags(write=False)
    return X, C


def rows_case(run, launches=(), write_bw=True):
    X, C = rows_spectra()
    k_of = crt_index()
    Xs = np.empty((K1, K2, 2 * K3), dtype=np.uint32)  # every row doubled
    Xs[:, :, :K3] = pack_h2(X[k_of])
    Xs[:, :, K3:] = Xs[:, :, :K3]
    Cs = pack_h2(C[:, :, k_of])
    n = len(run.bins)
    return [np.array([MAGIC, 2, n, run.gc, run.shift, NSLOTS, ROWS_GUARD, int(write_bw)], dtype=np.int64), Xs, Cs, np.array(run.bins, dtype=np.int32),
            np.array(run.slots, dtype=np.int64) * (2 * NP), launch_table(launches)]


def product_spectrum(s, slot):
    """Natural-order product spectrum of a cell rotated by s bins: Y_c[k] = X[(k - s) mod N] C_c[k] (C as stored: the library stores the
    conjugated code spectrum)."""
    X, C = rows_spectra()
    return np.roll(X, s)[None, :] * C[slot]


def rows_reference(s, slot):
    """[2][53][12][3125] over (component, k1, k2, t3): inverse 3125-point transform (unnormalised) of the product spectrum's rows."""
    return np.fft.ifft(product_spectrum(s, slot)[:, crt_index()], axis=-1) * K3


def direct_row(s, slot, c, k1, k2, t3):
    Y = product_spectrum(s, slot)[c, crt_index()[k1, k2]]
    return np.sum(Y * np.exp(2j * np.pi * ((np.arange(K3) * t3) % K3) / K3))


def e2e_reference(s, slot):
    """a[lag] = w0 |y_d| + w1 |y_p| with y_c = the N-point inverse transform of the natural-order product spectrum."""
    y = np.fft.ifft(product_spectrum(s, slot), axis=-1) * NP
    return W0 * np.abs(y[0]) + W1 * np.abs(y[1])


def storage_tolerance(ref, c):
    """Per real component of an fp16-stored transform output: fp16 rounding of a normal (2^-11 |ref|) or subnormal (2^-25) value
    + c x the row's largest |ref| for the fp32 transform (rows along the last axis)."""
    rowmax = np.max(np.abs(ref), axis=-1, keepdims=True)
    return 2.0 ** -11 * np.abs(ref.real) + 2.0 ** -25 + c * rowmax, 2.0 ** -11 * np.abs(ref.imag) + 2.0 ** -25 + c * rowmax


def measure_c(got, ref):
    """The smallest c of storage_tolerance that passes every component."""
    rowmax = np.max(np.abs(ref), axis=-1, keepdims=True)
    er = np.abs(got.real - ref.real) - 2.0 ** -11 * np.abs(ref.real) - 2.0 ** -25
    ei = np.abs(got.imag - ref.imag) - 2.0 ** -11 * np.abs(ref.imag) - 2.0 ** -25
    return max(0.0, float(np.max(er / rowmax)), float(np.max(ei / rowmax)))


# ---- column pass ----------------------------------------------------------------------------------------------------------------
class ColsCell:
    """One cell of the inter-pass buffer with its float64 reference: m[c][t1][t2][t3] = |y_c|^2 and a = w0 |y_d| + w1 |y_p| in grid
    order [53][12][3125], both from the ROUNDED buffer."""

    def __init__(self, name, z, claims=0, notes=None):
        self.name = name
        self.words = bw_pack(z)
        y = np.fft.ifft2(z, axes=(1, 2)) * (K1 * K2)
        self.m = y.real ** 2 + y.imag ** 2
        self.a = W0 * np.sqrt(self.m[0]) + W1 * np.sqrt(self.m[1])
        self.max = float(self.a.max())
        self.claims = claims  # lags at or above KEEP (1 + BAND) x the cell's own maximum the case claims to have, at least
        self.notes = notes or {}
        for arr in (self.words, self.m, self.a):
            arr.setflags(write=False)

    def value_tolerance(self, eps, idx=None):
        """Per lag (grid order; idx = flat grid positions, default all): the kernel forms |y|^2 of the pair (t2, 12 - t2) as S +- X,
        so the error of |y_c|^2 scales with S_c = |y_c[t2]|^2 + |y_c[12 - t2]|^2, not with the output:
        sum_c w_c (sqrt(m_c + eps S_c) - sqrt(m_c)) + 1e-6 a."""
        m = self.m.reshape(2, -1)
        if idx is None:
            idx = np.arange(NP)
        t1, rem = np.divmod(idx, K2 * K3)
        t2, t3 = np.divmod(rem, K3)
        mirror = (t1 * K2 + (K2 - t2) % K2) * K3 + t3
        mc = m[:, idx]
        grow = np.sqrt(mc + eps * (mc + m[:, mirror])) - np.sqrt(mc)
        return W0 * grow[0] + W1 * grow[1] + 1e-6 * self.a.reshape(-1)[idx]

    def measure_eps(self, got_grid):
        """The smallest eps of value_tolerance that passes every lag (bisection; got_grid in grid order)."""
        a = self.a.reshape(-1)
        err = np.abs(got_grid - a)
        idx = np.nonzero(err > 1e-6 * a)[0]
        if not len(idx):
            return 0.0
        lo, hi = 0.0, 1e-6
        while np.any(err[idx] > self.value_tolerance(hi, idx)):
            lo, hi = hi, hi * 4
            if hi > 1.0:
                return float("inf")
        for _ in range(30):
            mid = 0.5 * (lo + hi)
            if np.any(err[idx] > self.value_tolerance(mid, idx)):
                lo = mid
            else:
                hi = mid
        return hi


def direct_col(words, c, t1, t2, t3):
    """y_c[t1, t2, t3] as a direct 636-term sum over the packed cell, addressed through bw_piece."""
    k1, k2 = np.meshgrid(np.arange(K1), np.arange(K2), indexing="ij")
    z = unpack_h2(np.asarray(words)[bw_piece(k1 // 2, k2, t3) + 2 * c + (k1 & 1)])
    return np.sum(z * np.exp(2j * np.pi * (((k1 * t1) % K1) / K1 + ((k2 * t2) % K2) / K2)))


def spectrum_of(y):
    """Lag domain -> the fp16-rounded buffer values z[2][53][12][3125]."""
    return round_h2(np.fft.fft2(y, axes=(1, 2)) / (K1 * K2))


def noise_floor(rng, sigma):
    return sigma * (rng.standard_normal((2, K1, K2, K3)) + 1j * rng.standard_normal((2, K1, K2, K3))) * np.sqrt(0.5)


def plant(y, rng, t1, t2, t3, a, add=False):
    """Lag (t1, t2, t3) takes the sieve value a: components in the ratio w0 : w1 (the Cauchy-Schwarz bound of the kernel is then
    tight), random phases."""
    ph = np.exp(2j * np.pi * rng.random(2))
    v = np.array([W0, W1]) * a / WSUM2 * ph
    if add:
        y[:, t1, t2, t3] += v
    else:
        y[:, t1, t2, t3] = v


def shares_lane(p, q):
    """Do outputs p, q = (t1, t2, t3) sit in one lane of the column pass?  A lane holds one t3, the t1 of one residue mod 8 (one per
    output block) and t2 = 0..5 (even lane) or 6..11 (odd lane)."""
    return p[2] == q[2] and p[0] % 8 == q[0] % 8 and (p[1] < 6) == (q[1] < 6)


@functools.lru_cache(maxsize=None)
def cell_peaks():
    """Value mode: a noise floor with 40 peaks of 50..1000 times its level on top."""
    rng = np.random.default_rng(101)
    y = noise_floor(rng, 1.0)
    for _ in range(40):
        plant(y, rng, rng.integers(K1), rng.integers(K2), rng.integers(K3), 50.0 * 20.0 ** rng.random(), add=True)
    return ColsCell("peaks", spectrum_of(y))


EDGE_T1, EDGE_T2, EDGE_T3 = (0, 52), (0, 5, 6, 7, 11), (0, 15, 16, 3119, 3120, 3124)


@functools.lru_cache(maxsize=None)
def cell_edges():
    """Value mode: peaks on every edge -- the first and last t1; t2 = 0 and 6 (the separate S0 / S6 path), 5 and 7 (one lane pair),
    11; the first and last lag of a tile, of the last full tile (3119), and the 5-lag last tile (3120..3124)."""
    rng = np.random.default_rng(102)
    y = noise_floor(rng, 0.25)
    n = 0
    for t1 in EDGE_T1:
        for t2 in EDGE_T2:
            for t3 in EDGE_T3:
                plant(y, rng, t1, t2, t3, 100.0 + 7.0 * n)
                n += 1
    return ColsCell("edges", spectrum_of(y), notes={"peaks": n})


@functools.lru_cache(maxsize=None)
def cell_noise():
    """Sieve mode: noise only."""
    return ColsCell("noise", spectrum_of(noise_floor(np.random.default_rng(103), 1.0)), claims=1)


NEAR_LOW, NEAR_HIGH = 120, 180


@functools.lru_cache(maxsize=None)
def cell_near():
    """Sieve mode: 300 planted peaks between 0.990 and 1.0 of the maximum, none between 0.9958 and 0.9962 of it (the threshold is
    0.996: the band stays empty), among them 8 lane-sharing pairs above the threshold (the exhaustive pass) and 4 pairs across it; one of
    the pairs sits in the 5-lag last tile and one single peak above the threshold at t3 = 3124, whose wave has three masked lags."""
    rng = np.random.default_rng(104)
    y = noise_floor(rng, 1.0)
    A = 2000.0
    low = list(np.linspace(0.990, 0.9958, NEAR_LOW))
    high = list(np.linspace(0.9962, 1.0, NEAR_HIGH))
    rng.shuffle(low)
    rng.shuffle(high)
    used, pairs = set(), []

    def fresh(t3=None, like=None):
        while True:
            if like is None:
                p = (int(rng.integers(K1)), int(rng.integers(K2)), int(rng.integers(K3)) if t3 is None else t3)
            else:  # another output of the same lane
                p = ((like[0] % 8 + 8 * int(rng.integers(7))) % 56, int(rng.integers(6)) + (0 if like[1] < 6 else 6), like[2])
            if p[0] < K1 and p not in used and p != like:
                used.add(p)
                return p

    for i in range(12):
        p = fresh(t3=3123 if i == 0 else None)  # one pair in the 5-lag last tile
        q = fresh(like=p)
        plant(y, rng, *p, A * high.pop())
        plant(y, rng, *q, A * (high.pop() if i < 8 else low.pop()))
        pairs.append((p, q, i < 8))
    for j, f in enumerate(high + low):  # (the first of them, above the threshold, at the last lag t3: alone in its lane)
        plant(y, rng, *fresh(t3=K3 - 1 if j == 0 else None), A * f)
    return ColsCell("near", spectrum_of(y), claims=NEAR_HIGH, notes={"pairs": pairs})


TIE_T3 = 1234
TIE_VALUE = 3.0 - 2.0j


@functools.lru_cache(maxsize=None)
def cell_tie():
    """Sieve mode: at one t3 only (k1, k2) = (0, 0) is non-zero: all 636 outputs of that t3 are that value -- exactly, in float64 and in
    the kernel's fp32 (the coefficient of k1 = 0 is 1 with a zero lo part; the 12-point stage adds zeros) -- and the cell's maximum
    over a small noise floor.  cellmax must name the smallest of the 636 lags, and all of them are listed."""
    rng = np.random.default_rng(105)
    z = spectrum_of(noise_floor(rng, 0.05))
    z[:, :, :, TIE_T3] = 0.0
    z[:, 0, 0, TIE_T3] = TIE_VALUE
    return ColsCell("tie", z, claims=K1 * K2, notes={"t3": TIE_T3})


def coef_parts(t1):
    """(c_hi, s_hi, c_lo, s_lo)[k1] of output t1 of the 53-point stage, as make_coef_frags splits them: hi = fp16(fp32(v)),
    lo = fp16(fp32(v - hi))."""
    ang = 2.0 * np.pi * ((np.arange(K1) * t1) % K1) / K1

    def split(v):
        hi = v.astype(np.float32).astype(np.float16).astype(np.float64)
        return hi, (v - hi).astype(np.float32).astype(np.float16).astype(np.float64)

    ch, cl = split(np.cos(ang))
    sh, sl = split(np.sin(ang))
    return ch, sh, cl, sl


def hi_only_bound(z_wave):
    """What the bound pass of the shipped kernel sees of the lags of one wave (z_wave[2][53][12][4]: their buffer values) WITHOUT its
    analytic margin: the largest sqrt(|y_d|^2 + |y_p|^2) with the 53-point coefficients rounded to fp16 (float64 arithmetic otherwise)."""
    T = np.empty((K1, K1), dtype=np.complex128)
    for t1 in range(K1):
        ch, sh, _, _ = coef_parts(t1)
        T[t1] = ch + 1j * sh
    u = np.einsum("tk,ckql->ctql", T, z_wave)
    y = np.fft.ifft(u, axis=2) * K2
    return float(np.sqrt(np.max(np.sum(np.abs(y) ** 2, axis=0))))


ADV_T3, ADV_T2 = 2002, 5
ADV_PEAK = (7, 3, 5, 1000.0)
ADV_ABOVE = 1e-4  # the adversarial output sits at KEEP (1 + ADV_ABOVE) of the maximum


@functools.lru_cache(maxsize=None)
def cell_adversarial():
    """Sieve mode, for the hi-only bound.  A peak in tile 0 sets the threshold.  At t3 = ADV_T3 (tile 125, its own wave: lags
    2000..2003) the 53 inputs of each k2 are alpha conj(W53^(k1 t1)) + m (sgn c_lo[k1] - j sgn s_lo[k1]) for one output t1: the second
    term is signed like the lo parts of that output's coefficients, so all 106 lo products add up in its real part, in line with the
    53 alpha of the first term -- the hi-only estimate of that output undershoots most.  Scaled so that the output sits ADV_ABOVE
    above the threshold: it must be listed, and without the margin `dlt` the bound pass would skip its wave (hi_only_bound)."""
    rng = np.random.default_rng(106)
    y = noise_floor(rng, 1.0)
    plant(y, rng, *ADV_PEAK)
    z = spectrum_of(y)
    big = ColsCell("tmp", z).max
    g = np.exp(-2j * np.pi * ((np.arange(K2) * ADV_T2) % K2) / K2) / K2
    k1 = np.arange(K1)
    best = None
    for t1 in range(1, K1):
        ch, sh, cl, sl = coef_parts(t1)
        x1 = 0.7 * np.exp(-2j * np.pi * ((k1 * t1) % K1) / K1) + (np.sign(cl) - 1j * np.sign(sl))
        u_hi = np.array([np.sum((coef_parts(t)[0] + 1j * coef_parts(t)[1]) * x1) for t in range(K1)])
        u = np.sum((ch + cl + 1j * (sh + sl)) * x1)
        gain = abs(u) / abs(u_hi[t1]) - 1.0  # the undershoot of the target
        others = np.max(np.abs(np.delete(u_hi, t1))) / abs(u)
        if others < 0.9 and (best is None or gain > best[0]):
            best = (gain, t1, x1)
    _, t1, x1 = best
    col = np.array([W0, W1])[:, None, None] / WSUM2 * x1[None, :, None] * g[None, None, :]
    scale = KEEP * (1.0 + ADV_ABOVE) * big / abs(np.sum(np.exp(2j * np.pi * ((k1 * t1) % K1) / K1) * x1))
    for _ in range(6):  # (the fp16 rounding of the column moves the output by ~1e-5 of itself: settle on the rounded buffer)
        z[:, :, :, ADV_T3] = round_h2(scale * col)
        yy = np.fft.ifft2(z[:, :, :, ADV_T3], axes=(1, 2)) * (K1 * K2)
        a = W0 * abs(yy[0, t1, ADV_T2]) + W1 * abs(yy[1, t1, ADV_T2])
        r = a / (KEEP * (1.0 + ADV_ABOVE) * big)
        if abs(r - 1.0) < 1e-5:
            break
        scale /= r
    t0 = ADV_T3 // 4 * 4
    return ColsCell("adversarial", z, claims=2, notes={"target": (t1, ADV_T2, ADV_T3), "gain": best[0], "z_wave": z[:, :, :, t0:t0 + 4].copy()})


# The cells of the multi-cell launches, in launch order; with cell0 = 3 and lb_div = 2 the run-wide cells 3 | 4 5 | 6 7 share a bound:
# `near` alone (with a cell that is not of the launch), `noise` with `tie`, `adversarial` with `peaks`.
MULTI_CELLS = (cell_near, cell_noise, cell_tie, cell_adversarial, cell_peaks)
MULTI_CELL0, MULTI_LB_DIV = 3, 2
MULTI_NCELLS, MULTI_QCHUNK = (1, 2, 5), (1, 4, 8)


def multi_grids(ncells, qchunk):
    """7 and 512 (smaller and larger than qchunk x ncells, neither divides the item count), the host's own formula, one workgroup per item."""
    return (7, 512, host_grid(ncells, qchunk), items_of(ncells, qchunk))


def multi_launches():
    return [Launch(n, MULTI_CELL0, MULTI_LB_DIV, q, g, 1 << 16, True, KEEP) for n in MULTI_NCELLS for q in MULTI_QCHUNK for g in multi_grids(n, q)]


def group_maxima(cells, cell0, lb_div):
    """Per cell of a launch: the largest reference maximum among the launch's cells that share its lb slot."""
    slot = [(cell0 + i) // lb_div for i in range(len(cells))]
    return [max(c.max for c, s in zip(cells, slot) if s == slot[i]) for i in range(len(cells))]


def required_and_band(cell, gmax, keep=KEEP):
    """(grid positions of the lags the list must hold, number of lags in the ambiguity band of the threshold keep x gmax)."""
    a = cell.a.reshape(-1)
    thr = keep * gmax
    return np.nonzero(a >= thr * (1.0 + BAND))[0], int(np.count_nonzero(np.abs(a - thr) <= BAND * thr))


def cols_case(cells, launches):
    return [np.array([MAGIC, 3, len(cells)], dtype=np.int64), np.concatenate([c.words for c in cells]), launch_table(launches)]
