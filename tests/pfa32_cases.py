"""Inputs and float64 references for the stages of the N-point search pair at 53 MS/s (csrc/bds_acq_pfa32.h: N = 1 060 000 =
53 x 32 x 625), shared by tests/test_pfa32_cases.py (the CPU checks of the cases themselves) and tests/test_pfa32_stages_gpu.py (the
kernels, through tools/probe/pfa32_stages.hip).  The size-free helpers -- fp16 packing, the case-file format, the launch table, the
result parser, the tolerance forms -- are those of tests/pfa_cases.py; everything that knows a size is defined here.

NumPy only.  Every reference is numpy.fft in float64 over the Good-Thomas index maps of the header:
  spectrum index k <-> (k1, k2, k3) = (k mod 53, k mod 32, k mod 625),   lag_of(t1, t2, t3) = (t1 N/53 + t2 N/32 + t3 N/625) mod N,
  bw_piece(mp, k2, t3) for the tiled inter-pass buffer (tiles of 8 lags; the last tile holds the single lag 624).
Column-pass inputs are built in the LAG domain and the reference is computed from the ROUNDED buffer, as in tests/pfa_cases.py.
"""
import functools
from collections import namedtuple

import numpy as np

from pfa_cases import (BAND, EXTRA_DT, GUARD_EXTRA, GUARD_WORD, KEEP, MAGIC, W0, W1, WSUM2, Launch, group_maxima, guard_intact,  # noqa: F401
                       launch_table, measure_c, pack_h2, parse_cols, plant, read_arrays, round_h2, storage_tolerance, unpack_h2, write_arrays)

K1, K2, K3 = 53, 32, 625
NP = K1 * K2 * K3  # 1 060 000
MP = 27
TILE = 8
TILES = (K3 + TILE - 1) // TILE  # 79
CELL_ELEMS = TILES * MP * K2 * TILE * 4
WAVE_LAGS = 2                            # lags t3 of a wave item of the column pass
WAVE_ITEMS_PER_CELL = (K3 + 1) // 2      # waves with t0 = 8 tile + 2 wave < 625: 313
NBLOCKS = 7                              # output blocks of a wave item


# ---- index maps ----------------------------------------------------------------------------------------------------------------
def lag_of(t1, t2, t3):
    t1, t2, t3 = (np.asarray(v, dtype=np.int64) for v in (t1, t2, t3))
    return (t1 * (NP // K1) + t2 * (NP // K2) + t3 * (NP // K3)) % NP


def bw_piece(mp, k2, t3):
    """Element index (fp16 complex, 4 bytes) of the 4-element piece of (mp, k2, t3) in its cell."""
    return ((t3 // TILE * MP + mp) * K2 + k2) * (TILE * 4) + (t3 % TILE) * 4


@functools.lru_cache(maxsize=None)
def crt_index():
    """k_of[k1, k2, k3] = the natural index k with (k mod 53, k mod 32, k mod 625) = (k1, k2, k3)."""
    k = np.arange(NP, dtype=np.int64)
    k_of = np.empty((K1, K2, K3), dtype=np.int64)
    k_of[k % K1, k % K2, k % K3] = k
    k_of.setflags(write=False)
    return k_of


@functools.lru_cache(maxsize=None)
def lag_grid():
    """(lag[t1, t2, t3], its inverse: grid position (flat index into [53][32][625]) of every lag)."""
    lag = lag_of(np.arange(K1)[:, None, None], np.arange(K2)[None, :, None], np.arange(K3)[None, None, :])
    inv = np.empty(NP, dtype=np.int64)
    inv[lag.ravel()] = np.arange(NP, dtype=np.int64)
    lag.setflags(write=False)
    inv.setflags(write=False)
    return lag, inv


def bw_pack(z):
    """z[2][53][32][625] (fp16-exact values) -> a cell of the inter-pass buffer.  The pad row k1 = 53 is zero, as the row pass leaves it;
    the 7 pad lags of the last tile hold 0xffffffff (two fp16 NaNs): no kernel may read them."""
    full = np.full((2, 2 * MP, K2, TILES * TILE), 0xFFFFFFFF, dtype=np.uint32)
    full[:, :K1, :, :K3] = pack_h2(z)
    full[:, K1, :, :K3] = 0
    # (c, mp, row, k2, tile, lag) -> [tile][mp][k2][lag][c][row]
    return np.ascontiguousarray(full.reshape(2, MP, 2, K2, TILES, TILE).transpose(4, 1, 3, 5, 0, 2)).reshape(-1)


def bw_unpack_words(cell):
    """A cell of the inter-pass buffer -> its words as [2][54][32][632] (pad row and pad lags included)."""
    w = np.asarray(cell, dtype=np.uint32).reshape(TILES, MP, K2, TILE, 2, 2)
    return np.ascontiguousarray(w.transpose(4, 1, 5, 2, 0, 3)).reshape(2, 2 * MP, K2, TILES * TILE)


def items_of(ncells, qchunk):
    return (TILES + qchunk - 1) // qchunk * qchunk * ncells


def host_grid(ncells, qchunk):
    """The column grid csrc/bds_acq.hip launches for a cell list of this size."""
    items = items_of(ncells, qchunk)
    return min(items, max(512, min(8192, items // 24)))


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
    """fft(x) * scale in the CRT layout [batch][53][32][625] (not conjugated)."""
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
RowsRun = namedtuple("RowsRun", "name bins slots gc shift")
# Rotations s = bin * shift in {0, 1, 31, 32, 33, 52, 53, 200, 624, 625, 640}: 0, the first step, around the periods of the 32-, the 53- and
# the 625-point dimension, the last bin of the default band.  Chunks of two with a short last chunk, the PRN slot changing from chunk to
# chunk (cs[c0] serves the whole chunk); then one cell per chunk; then shift 2 (rotations 624, 0, 640).
ROWS_RUNS = (
    RowsRun("gc2", (0, 1, 31, 32, 33), (0, 0, 1, 1, 0), 2, 1),
    RowsRun("gc1", (52, 53, 200, 624, 625), (1, 0, 1, 0, 1), 1, 1),
    RowsRun("shift2", (312, 0, 320), (0, 0, 1), 2, 2),
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
    """Natural-order product spectrum of a cell rotated by s bins: Y_c[k] = X[(k - s) mod N] C_c[k] (C as stored)."""
    X, C = rows_spectra()
    return np.roll(X, s)[None, :] * C[slot]


def rows_reference(s, slot):
    """[2][53][32][625] over (component, k1, k2, t3): inverse 625-point transform (unnormalised) of the product spectrum's rows."""
    return np.fft.ifft(product_spectrum(s, slot)[:, crt_index()], axis=-1) * K3


def direct_row(s, slot, c, k1, k2, t3):
    Y = product_spectrum(s, slot)[c, crt_index()[k1, k2]]
    return np.sum(Y * np.exp(2j * np.pi * ((np.arange(K3) * t3) % K3) / K3))


def e2e_reference(s, slot):
    """a[lag] = w0 |y_d| + w1 |y_p| with y_c = the N-point inverse transform of the natural-order product spectrum."""
    y = np.fft.ifft(product_spectrum(s, slot), axis=-1) * NP
    return W0 * np.abs(y[0]) + W1 * np.abs(y[1])


# ---- column pass ----------------------------------------------------------------------------------------------------------------
class ColsCell:
    """One cell of the inter-pass buffer with its float64 reference: m[c][t1][t2][t3] = |y_c|^2 and a = w0 |y_d| + w1 |y_p| in grid
    order [53][32][625], both from the ROUNDED buffer."""

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
        """Per lag (grid order; idx = flat grid positions, default all), the form of tests/pfa_cases.py:
        sum_c w_c (sqrt(m_c + eps S_c) - sqrt(m_c)) + 1e-6 a with S_c = |y_c[t2]|^2 + |y_c[32 - t2]|^2."""
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
    """y_c[t1, t2, t3] as a direct 1696-term sum over the packed cell, addressed through bw_piece."""
    k1, k2 = np.meshgrid(np.arange(K1), np.arange(K2), indexing="ij")
    z = unpack_h2(np.asarray(words)[bw_piece(k1 // 2, k2, t3) + 2 * c + (k1 & 1)])
    return np.sum(z * np.exp(2j * np.pi * (((k1 * t1) % K1) / K1 + ((k2 * t2) % K2) / K2)))


def spectrum_of(y):
    """Lag domain -> the fp16-rounded buffer values z[2][53][32][625]."""
    return round_h2(np.fft.fft2(y, axes=(1, 2)) / (K1 * K2))


def noise_floor(rng, sigma):
    return sigma * (rng.standard_normal((2, K1, K2, K3)) + 1j * rng.standard_normal((2, K1, K2, K3))) * np.sqrt(0.5)


def lane_of(p):
    """The lane of the column pass that ends with output p = (t1, t2, t3): (t3, t1 mod 8, t2 mod 2, t2 >= 16) -- a lane holds one t3, the
    t1 of one residue mod 8 (one per output block), and the 8 t2 = e + 2 tai + 16 h + 4 tbi of one parity e and one half h."""
    return (p[2], p[0] % 8, p[1] % 2, p[1] >= 16)


def shares_lane(p, q):
    return lane_of(p) == lane_of(q)


@functools.lru_cache(maxsize=None)
def cell_noise():
    """Value and sieve mode: noise only."""
    return ColsCell("noise", spectrum_of(noise_floor(np.random.default_rng(103), 1.0)), claims=1)


EDGE_T1, EDGE_T2 = (0, 52), (0, 1, 15, 16, 17, 31)
EDGE_T3 = (0, 1, 2, 7, 8, 615, 616, 622, 623, 624)  # first / last t3; both sides of a wave's pair (0 | 1, 622 | 623), of two waves (1 | 2) and of tiles (7 | 8, 615 | 616, 623 | 624)


@functools.lru_cache(maxsize=None)
def cell_edges():
    """Value mode: peaks on every edge -- the first and last t1; t2 = 0, 1 (the lane pair's split of the ta), 15 | 16 | 17 (the split of
    the 32 between the two 16-lane rows), 31; t3 on both sides of every boundary of the layout (EDGE_T3)."""
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
    of the pairs sits at t3 = 623 (the last pair of lags of the last full tile) and one single peak above the threshold at t3 = 624, whose
    wave has one masked lag."""
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
                p = ((like[0] % 8 + 8 * int(rng.integers(7))) % 56, like[1] % 2 + 2 * int(rng.integers(8)) + (16 if like[1] >= 16 else 0), like[2])
            if p[0] < K1 and p not in used and p != like:
                used.add(p)
                return p

    for i in range(12):
        p = fresh(t3=623 if i == 0 else None)
        q = fresh(like=p)
        assert shares_lane(p, q)
        plant(y, rng, *p, A * high.pop())
        plant(y, rng, *q, A * (high.pop() if i < 8 else low.pop()))
        pairs.append((p, q, i < 8))
    for j, f in enumerate(high + low):  # (the first of them, above the threshold, at the last lag t3: alone in its tile)
        plant(y, rng, *fresh(t3=K3 - 1 if j == 0 else None), A * f)
    return ColsCell("near", spectrum_of(y), claims=NEAR_HIGH, notes={"pairs": pairs})


TIE_T3 = 234
TIE_VALUE = 3.0 - 2.0j


@functools.lru_cache(maxsize=None)
def cell_tie():
    """Sieve mode: at one t3 only (k1, k2) = (0, 0) is non-zero: all 1696 outputs of that t3 are that value -- exactly, in float64 and in
    the kernel's fp32 (the coefficient of k1 = 0 is 1 with a zero lo part; the 32-point stage adds zeros and multiplies by unit twiddles
    whose products with a lone value are rounded the same way in every lane that holds the same ta) -- over a small noise floor."""
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
    """7 and 512 (smaller and larger than qchunk x ncells, neither divides the item count), the host's own formula, one workgroup per item."""
    return (7, 512, host_grid(ncells, qchunk), items_of(ncells, qchunk))


def multi_launches():
    return [Launch(n, MULTI_CELL0, MULTI_LB_DIV, q, g, 1 << 16, True, KEEP) for n in MULTI_NCELLS for q in MULTI_QCHUNK for g in multi_grids(n, q)]


def required_and_band(cell, gmax, keep=KEEP):
    """(grid positions of the lags the list must hold, number of lags in the ambiguity band of the threshold keep x gmax)."""
    a = cell.a.reshape(-1)
    thr = keep * gmax
    return np.nonzero(a >= thr * (1.0 + BAND))[0], int(np.count_nonzero(np.abs(a - thr) <= BAND * thr))


def cols_case(cells, launches):
    return [np.array([MAGIC, 3, len(cells)], dtype=np.int64), np.concatenate([c.words for c in cells]), launch_table(launches)]
