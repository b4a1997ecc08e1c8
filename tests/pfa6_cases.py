"""Inputs and float64 references for the stages of the opt-in N-point search pair for B2a at 99.375 MS/s (csrc/bds_acq_pfa6.h: N = 198 750 =
53 x 6 x 625), shared by tests/test_pfa6_cases.py (the CPU checks of the cases themselves) and tests/test_pfa6_stages_gpu.py (the kernels,
through tools/probe/pfa6_stages.hip).  The size-free helpers -- fp16 packing, the case-file format, the result parser, the tolerance
forms -- are those of tests/pfa_cases.py; everything that knows a size is defined here.

NumPy only.  Every reference is numpy.fft in float64 over the Good-Thomas index maps of the header:
  spectrum index k <-> (k1, k2, k3) = (k mod 53, k mod 6, k mod 625),   lag_of(t1, t2, t3) = (t1 N/53 + t2 N/6 + t3 N/625) mod N,
  bw_piece(mp, k2, t3) for the tiled inter-pass buffer (tiles of 32 lags; the last tile holds the 17 lags 608..624),
  Doppler bin b = q m + j -> signal spectrum j rotated by p m (acqStep N / fs = p / q in lowest terms).
Column-pass inputs are built in the LAG domain and the reference is computed from the ROUNDED buffer, as in tests/pfa_cases.py.
B2a weighs both components with 1 (B2a/acquisition.m:208-209): W0 = W1 = 1 here, where the B1C cases carry sqrt(11 / 40), sqrt(29 / 40).
"""
import functools
from collections import namedtuple

import numpy as np

from pfa_cases import (BAND, EXTRA_DT, GUARD_EXTRA, GUARD_WORD, KEEP, MAGIC, group_maxima, guard_intact, measure_c, pack_h2,  # noqa: F401
                       parse_cols, read_arrays, round_h2, storage_tolerance, unpack_h2, write_arrays)

K1, K2, K3 = 53, 6, 625
NP = K1 * K2 * K3  # 198 750
MP = 27
TILE = 32
TILES = (K3 + TILE - 1) // TILE  # 20
CELL_ELEMS = TILES * MP * K2 * TILE * 4
WAVE_LAGS = 8                            # lags t3 of a wave item of the column pass
WAVE_ITEMS_PER_CELL = 19 * 4 + 3         # waves with t0 = 32 tile + 8 wave < 625
NBLOCKS = 7                              # output blocks of a wave item
MAX_Q = 5
W0 = W1 = 1.0
WSUM2 = 2.0
FS = 99.375e6


# ---- index maps ----------------------------------------------------------------------------------------------------------------
def lag_of(t1, t2, t3):
    t1, t2, t3 = (np.asarray(v, dtype=np.int64) for v in (t1, t2, t3))
    return (t1 * (NP // K1) + t2 * (NP // K2) + t3 * (NP // K3)) % NP


def bw_piece(mp, k2, t3):
    """Element index (fp16 complex, 4 bytes) of the 4-element piece of (mp, k2, t3) in its cell."""
    return ((t3 // TILE * MP + mp) * K2 + k2) * (TILE * 4) + (t3 % TILE) * 4


@functools.lru_cache(maxsize=None)
def crt_index():
    """k_of[k1, k2, k3] = the natural index k with (k mod 53, k mod 6, k mod 625) = (k1, k2, k3)."""
    k = np.arange(NP, dtype=np.int64)
    k_of = np.empty((K1, K2, K3), dtype=np.int64)
    k_of[k % K1, k % K2, k % K3] = k
    k_of.setflags(write=False)
    return k_of


@functools.lru_cache(maxsize=None)
def lag_grid():
    """(lag[t1, t2, t3], its inverse: grid position (flat index into [53][6][625]) of every lag)."""
    lag = lag_of(np.arange(K1)[:, None, None], np.arange(K2)[None, :, None], np.arange(K3)[None, None, :])
    inv = np.empty(NP, dtype=np.int64)
    inv[lag.ravel()] = np.arange(NP, dtype=np.int64)
    lag.setflags(write=False)
    inv.setflags(write=False)
    return lag, inv


def bw_pack(z):
    """z[2][53][6][625] (fp16-exact values) -> a cell of the inter-pass buffer.  The pad row k1 = 53 is zero, as the row pass leaves it;
    the 15 pad lags of the last tile hold 0xffffffff (two fp16 NaNs): no kernel may read them."""
    full = np.full((2, 2 * MP, K2, TILES * TILE), 0xFFFFFFFF, dtype=np.uint32)
    full[:, :K1, :, :K3] = pack_h2(z)
    full[:, K1, :, :K3] = 0
    # (c, mp, row, k2, tile, lag) -> [tile][mp][k2][lag][c][row]
    return np.ascontiguousarray(full.reshape(2, MP, 2, K2, TILES, TILE).transpose(4, 1, 3, 5, 0, 2)).reshape(-1)


def bw_unpack_words(cell):
    """A cell of the inter-pass buffer -> its words as [2][54][6][640] (pad row and pad lags included)."""
    w = np.asarray(cell, dtype=np.uint32).reshape(TILES, MP, K2, TILE, 2, 2)
    return np.ascontiguousarray(w.transpose(4, 1, 5, 2, 0, 3)).reshape(2, 2 * MP, K2, TILES * TILE)


def items_of(ncells, qchunk):
    return (TILES + qchunk - 1) // qchunk * qchunk * ncells


def host_grid(ncells, qchunk):
    """The column grid csrc/bds_acq.hip launches for a cell list of this size."""
    items = items_of(ncells, qchunk)
    return min(items, max(512, min(8192, items // 24)))


# A column launch of tools/probe/pfa6_stages.hip: the fields of pfa_cases.Launch + whether the masked kernel runs (ranges / src of the case)
Launch = namedtuple("Launch", "ncells cell0 lb_div qchunk grid extra_cap stats keep masked", defaults=(False,))


def launch_table(launches):
    return np.array([[l.ncells, l.cell0, l.lb_div, l.qchunk, l.grid, l.extra_cap, int(l.stats), l.keep, W0, W1, int(l.masked)] for l in launches],
                    dtype=np.float64).reshape(-1, 11)


# ---- the fractional Doppler step --------------------------------------------------------------------------------------------------
def step_ratio(step, fs, n=NP):
    """acqStep N / fs = p / q in lowest terms, in integers (pfa6::step_ratio); None when step or fs is no whole number of hertz."""
    from math import gcd

    if not (1 <= step <= 1e9 and 1 <= fs <= 1e12) or step != int(step) or fs != int(fs):
        return None
    a, b = int(step) * int(n), int(fs)
    g = gcd(a, b)
    return a // g, b // g


def admitted(step, fs, nbins, n=NP):
    """(p, q) when the pair takes this step (q <= 5, p >= 1, every rotation below N), else None: the rule of pfa6_pick in csrc/bds_acq.hip."""
    r = step_ratio(step, fs, n)
    if r is None or r[1] > MAX_Q or r[0] < 1 or r[0] * ((nbins + r[1] - 1) // r[1]) >= n:
        return None
    return r


def cell_of_bin(b, p, q):
    """0-based bin b = q m + j -> (spectrum index j, rotation p m)."""
    return b % q, (b // q) * p


def carrier(f, n=NP, fs=FS):
    """exp(+1i f phasePoints), phasePoints = n 2 pi / fs (B2a/acquisition.m:146, 199), f and fs whole hertz: the turn count reduced exactly."""
    k = np.arange(n, dtype=np.int64)
    return np.exp(2j * np.pi * ((int(f) * k) % int(fs)) / fs)


# ---- forward transforms ---------------------------------------------------------------------------------------------------------
FWD_SCALE = 1.0 / 65536.0
FWD_BATCH = 5


@functools.lru_cache(maxsize=None)
def forward_input():
    """Five integer-valued signals (exact in fp32, so the float64 reference sees what the kernel sees)."""
    rng = np.random.default_rng(11)
    x = np.round(20.0 * rng.standard_normal((FWD_BATCH, NP))) + 1j * np.round(3.0 * rng.standard_normal((FWD_BATCH, NP)))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def forward_reference():
    """fft(x) * scale in the CRT layout [batch][53][6][625] (not conjugated)."""
    X = np.fft.fft(forward_input(), axis=-1) * FWD_SCALE
    ref = X[:, crt_index()]
    ref.setflags(write=False)
    return ref


def forward_case(nb, doubled, conj, stride):
    x = forward_input()[:nb]
    xs = np.empty((nb, NP, 2), dtype=np.float32)
    xs[..., 0], xs[..., 1] = x.real, x.imag
    return [np.array([MAGIC, 1, nb, doubled, conj, stride], dtype=np.int64), np.array([FWD_SCALE]), xs]


def direct_npoint(x, k, sign):
    """sum_n x[n] exp(sign 2 pi j n k / N) of a natural-order x, one output k."""
    n = np.arange(NP, dtype=np.int64)
    w = np.exp(2j * np.pi * ((n * int(k)) % NP) / NP)
    return np.sum(x * (w if sign > 0 else np.conj(w)))


# ---- row pass -------------------------------------------------------------------------------------------------------------------
NSLOTS = 2
NSPEC = 5
RowsRun = namedtuple("RowsRun", "name bins slots gc p q")
# With p / q = 4 / 5 (cfg2) a bin b = 5 m + j reads spectrum j rotated by 4 m; with 1 / 1 the rotation is the bin.  The rotations cover 0,
# 1, around the periods of the 6- (5, 6, 7), the 53- (52, 53) and the 625-point dimension (624, 625) and one past it (640); the spectrum
# indices 0, 1 and 4.  Chunks of two with a short last chunk, the PRN slot changing from chunk to chunk (cs[c0] serves the whole chunk);
# then one cell per chunk.
ROWS_RUNS = (
    RowsRun("p1-gc2", (0, 1, 5, 6, 7), (0, 0, 1, 1, 0), 2, 1, 1),            # rotations 0, 1, 5, 6, 7 of spectrum 0
    RowsRun("p1-gc1", (52, 53, 624, 625, 640), (1, 0, 1, 0, 1), 1, 1, 1),    # rotations 52, 53, 624, 625, 640
    RowsRun("p4-gc2", (0, 1, 4, 65, 784), (0, 0, 1, 1, 0), 2, 4, 5),         # (spectrum, rotation) = (0, 0), (1, 0), (4, 0), (0, 52), (4, 624)
    RowsRun("p4-gc1", (6, 800, 781), (1, 0, 1), 1, 4, 5),                    # (1, 4), (0, 640), (1, 624)
)
ROWS_GUARD = TILE * MP * K2 * 4  # elements in front of and behind the destination: one tile


@functools.lru_cache(maxsize=None)
def rows_spectra():
    """(Xnat[spectrum][N], Cnat[slot][component][N]): fp16-exact spectra in natural order."""
    rng = np.random.default_rng(7)
    X = round_h2(8.0 * (rng.standard_normal((NSPEC, NP)) + 1j * rng.standard_normal((NSPEC, NP))))
    C = round_h2(0.125 * (rng.standard_normal((NSLOTS, 2, NP)) + 1j * rng.standard_normal((NSLOTS, 2, NP))))
    X.setflags(write=False)
    C.setflags(write=False)
    return X, C


def rows_case(run, launches=(), write_bw=True, rng=None, src=None):
    X, C = rows_spectra()
    k_of = crt_index()
    Xs = np.empty((NSPEC, K1, K2, 2 * K3), dtype=np.uint32)  # every row doubled
    Xs[..., :K3] = pack_h2(X[:, k_of])
    Xs[..., K3:] = Xs[..., :K3]
    Cs = pack_h2(C[:, :, k_of])
    n = len(run.bins)
    r, sc = mask_arrays(rng, n, src)
    return [np.array([MAGIC, 2, n, run.gc, run.p, run.q, NSLOTS, ROWS_GUARD, int(write_bw), NSPEC], dtype=np.int64), Xs, Cs, np.array(run.bins, dtype=np.int32),
            np.array(run.slots, dtype=np.int64) * (2 * NP), launch_table(launches), r, sc]


def mask_arrays(rng, n, src=None):
    """(int32 rng[n][4], int32 src[n]) of a case; no ranges: empty arrays"""
    if rng is None:
        return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
    r = np.asarray(rng, dtype=np.int32).reshape(n, 4)
    return r, (np.zeros(0, dtype=np.int32) if src is None else np.asarray(src, dtype=np.int32).reshape(n))


def product_spectrum(spec, s, slot):
    """Natural-order product spectrum of a cell: Y_c[k] = X_spec[(k - s) mod N] C_c[k] (C as stored)."""
    X, C = rows_spectra()
    return np.roll(X[spec], s)[None, :] * C[slot]


def rows_reference(spec, s, slot):
    """[2][53][6][625] over (component, k1, k2, t3): inverse 625-point transform (unnormalised) of the product spectrum's rows."""
    return np.fft.ifft(product_spectrum(spec, s, slot)[:, crt_index()], axis=-1) * K3


def direct_row(spec, s, slot, c, k1, k2, t3):
    Y = product_spectrum(spec, s, slot)[c, crt_index()[k1, k2]]
    return np.sum(Y * np.exp(2j * np.pi * ((np.arange(K3) * t3) % K3) / K3))


def e2e_reference(spec, s, slot):
    """a[lag] = w0 |y_d| + w1 |y_p| with y_c = the N-point inverse transform of the natural-order product spectrum."""
    y = np.fft.ifft(product_spectrum(spec, s, slot), axis=-1) * NP
    return W0 * np.abs(y[0]) + W1 * np.abs(y[1])


# ---- column pass ----------------------------------------------------------------------------------------------------------------
class ColsCell:
    """One cell of the inter-pass buffer with its float64 reference: m[c][t1][t2][t3] = |y_c|^2 and a = w0 |y_d| + w1 |y_p| in grid
    order [53][6][625], both from the ROUNDED buffer."""

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
        """Per lag (grid order; idx = flat grid positions, default all), the form of tests/pfa_cases.py: the kernel forms |y|^2 of the pair
        (t2, 6 - t2) as S +- X: sum_c w_c (sqrt(m_c + eps S_c) - sqrt(m_c)) + 1e-6 a with S_c = |y_c[t2]|^2 + |y_c[6 - t2]|^2."""
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
    """y_c[t1, t2, t3] as a direct 318-term sum over the packed cell, addressed through bw_piece."""
    k1, k2 = np.meshgrid(np.arange(K1), np.arange(K2), indexing="ij")
    z = unpack_h2(np.asarray(words)[bw_piece(k1 // 2, k2, t3) + 2 * c + (k1 & 1)])
    return np.sum(z * np.exp(2j * np.pi * (((k1 * t1) % K1) / K1 + ((k2 * t2) % K2) / K2)))


def spectrum_of(y):
    """Lag domain -> the fp16-rounded buffer values z[2][53][6][625]."""
    return round_h2(np.fft.fft2(y, axes=(1, 2)) / (K1 * K2))


def noise_floor(rng, sigma):
    return sigma * (rng.standard_normal((2, K1, K2, K3)) + 1j * rng.standard_normal((2, K1, K2, K3))) * np.sqrt(0.5)


def plant(y, rng, t1, t2, t3, a):
    """Lag (t1, t2, t3) takes the sieve value a: components in the ratio w0 : w1 (the Cauchy-Schwarz bound of the kernel is then tight),
    random phases."""
    ph = np.exp(2j * np.pi * rng.random(2))
    y[:, t1, t2, t3] = np.array([W0, W1]) * a / WSUM2 * ph


def lane_of(p):
    """The lane of the column pass that ends with output p = (t1, t2, t3): a lane holds the two lags t3 of one pair (t3 // 2), the t1 of one
    residue mod 8 (one per output block), and t2 = 0, 1, 2 (the even lane of the (re, im) pair) or 3, 4, 5 (the odd lane)."""
    return (p[2] // 2, p[0] % 8, p[1] >= 3)


def shares_lane(p, q):
    return lane_of(p) == lane_of(q)


@functools.lru_cache(maxsize=None)
def cell_noise():
    """Value and sieve mode: noise only."""
    return ColsCell("noise", spectrum_of(noise_floor(np.random.default_rng(103), 1.0)), claims=1)


EDGE_T1, EDGE_T2 = (0, 52), (0, 1, 3, 5)
# first / last t3; both sides of a lane's pair of lags (0 | 1), of a wave's 8 lags (7 | 8), of two tiles (31 | 32), of the last full tile
# (607 | 608), the last lag of the last tile's full waves (623) and the one live lag of its third wave (624)
EDGE_T3 = (0, 1, 7, 8, 31, 32, 607, 608, 615, 616, 623, 624)


@functools.lru_cache(maxsize=None)
def cell_edges():
    """Value mode: peaks on every edge -- the first and last t1; t2 = 0 and 3 (their own mirrors: the separate S0 / S3 path), 1 and 5 (one
    lane pair); t3 on both sides of every boundary of the layout (EDGE_T3)."""
    rng = np.random.default_rng(102)
    y = noise_floor(rng, 0.25)
    n = 0
    for t1 in EDGE_T1:
        for t2 in EDGE_T2:
            for t3 in EDGE_T3:
                plant(y, rng, t1, t2, t3, 100.0 + 7.0 * n)
                n += 1
    return ColsCell("edges", spectrum_of(y), notes={"peaks": n})


NEAR_LOW, NEAR_HIGH = 120, 180


@functools.lru_cache(maxsize=None)
def cell_near():
    """Sieve mode: 300 planted peaks between 0.990 and 1.0 of the maximum, none between 0.9958 and 0.9962 of it (the threshold is
    0.996: the band stays empty), among them 8 lane-sharing pairs above the threshold (the exhaustive listing) and 4 pairs across it; one
    of the pairs sits at t3 = 622 | 623 (the last lane of the last tile's second wave) and one single peak above the threshold at t3 = 624,
    whose wave has one live lag."""
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
                p = ((like[0] % 8 + 8 * int(rng.integers(7))) % 56, int(rng.integers(3)) + (3 if like[1] >= 3 else 0), like[2] // 2 * 2 + int(rng.integers(2)))
            if p[0] < K1 and p[2] < K3 and p not in used and p != like:
                used.add(p)
                return p

    for i in range(12):
        p = fresh(t3=623 if i == 0 else None)
        q = fresh(like=p)
        assert shares_lane(p, q)
        plant(y, rng, *p, A * high.pop())
        plant(y, rng, *q, A * (high.pop() if i < 8 else low.pop()))
        pairs.append((p, q, i < 8))
    for j, f in enumerate(high + low):  # (the first of them, above the threshold, at the last lag t3: alone in its wave)
        plant(y, rng, *fresh(t3=K3 - 1 if j == 0 else None), A * f)
    return ColsCell("near", spectrum_of(y), claims=NEAR_HIGH, notes={"pairs": pairs})


TIE_T3 = 234
TIE_VALUE = 3.0 - 2.0j


@functools.lru_cache(maxsize=None)
def cell_tie():
    """Sieve mode: at one t3 only (k1, k2) = (0, 0) is non-zero: all 318 outputs of that t3 are that value -- exactly, in float64 and in
    the kernel's fp32 (the coefficient of k1 = 0 is 1 with a zero lo part; the 6-point stage adds zeros) -- over a small noise floor."""
    rng = np.random.default_rng(105)
    z = spectrum_of(noise_floor(rng, 0.05))
    z[:, :, :, TIE_T3] = 0.0
    z[:, 0, 0, TIE_T3] = TIE_VALUE
    return ColsCell("tie", z, claims=K1 * K2, notes={"t3": TIE_T3})


# The cells of the multi-cell launches, in launch order; with cell0 = 3 and lb_div = 2 the run-wide cells 3 | 4 5 | 6 7 share a bound
MULTI_CELLS = (cell_near, cell_noise, cell_tie, cell_edges)
MULTI_CELL0, MULTI_LB_DIV = 3, 2
MULTI_NCELLS, MULTI_QCHUNK = (1, 2, 4), (1, 4, 8)


def multi_grids(ncells, qchunk):
    """7 and 512 (smaller and larger than qchunk x ncells), the host's own formula, one workgroup per item."""
    return (7, 512, host_grid(ncells, qchunk), items_of(ncells, qchunk))


def multi_launches():
    return [Launch(n, MULTI_CELL0, MULTI_LB_DIV, q, g, 1 << 16, True, KEEP) for n in MULTI_NCELLS for q in MULTI_QCHUNK for g in multi_grids(n, q)]


def required_and_band(cell, gmax, keep=KEEP, allowed=None):
    """(grid positions of the lags the list must hold, number of lags in the ambiguity band of the threshold keep x gmax); allowed: a
    boolean mask over the grid positions (the masked pass: only those lags are searched)."""
    a = cell.a.reshape(-1)
    if allowed is not None:
        a = np.where(allowed, a, -1.0)
    thr = keep * gmax
    return np.nonzero(a >= thr * (1.0 + BAND))[0], int(np.count_nonzero(np.abs(a - thr) <= BAND * thr))


def cols_case(cells, launches, rng=None, src=None, nlisted=None):
    """cells: the buffer's cells; a masked launch lists nlisted cells with ranges rng[nlisted][4] reading the buffer's cells src[nlisted]"""
    n = len(cells) if nlisted is None else nlisted
    r, s = mask_arrays(rng, n, src)
    return [np.array([MAGIC, 3, len(cells)], dtype=np.int64), np.concatenate([c.words for c in cells]), launch_table(launches), r, s]


# ---- masked mode ----------------------------------------------------------------------------------------------------------------
def in_ranges(rng4):
    """Boolean mask over the GRID positions [53 x 6 x 625] of the lags inside (lo1..hi1) or (lo2..hi2), inclusive, natural lag order."""
    lag = lag_grid()[0].ravel()
    lo1, hi1, lo2, hi2 = (int(v) for v in rng4)
    return ((lag >= lo1) & (lag <= hi1)) | ((lag >= lo2) & (lag <= hi2))


MASK_PEAKS = ((5, 1, 100), (30, 4, 333), (17, 2, 608), (44, 0, 9), (2, 5, 31), (51, 3, 624))


@functools.lru_cache(maxsize=None)
def cell_masked():
    """Masked mode: six peaks of 1000 .. 1500 over a floor of 1, the largest first; the ranges of MASK_RANGES put their edges on them."""
    rng = np.random.default_rng(107)
    y = noise_floor(rng, 1.0)
    for i, (t1, t2, t3) in enumerate(MASK_PEAKS):
        plant(y, rng, t1, t2, t3, 1500.0 - 100.0 * i)
    return ColsCell("masked", spectrum_of(y), notes={"lags": [int(lag_of(*p)) for p in MASK_PEAKS]})


def mask_ranges():
    """Per listed cell (lo1, hi1, lo2, hi2) on the peaks' lags L0 < L1 < .. (sorted): range 1 = [La, Lb] with both edges ON a peak
    (inclusive at lo and hi), range 2 starting one lag BEHIND a peak and ending one lag in FRONT of the next (both just outside); then the
    mirror case; one list entry with an empty first range; one with both ranges empty."""
    L = sorted(cell_masked().notes["lags"])
    return [(L[0], L[1], L[2] + 1, L[3] - 1),
            (L[1] + 1, L[2] - 1, L[4], L[5]),
            (1, 0, L[3], L[3]),
            (1, 0, 1, 0)]
