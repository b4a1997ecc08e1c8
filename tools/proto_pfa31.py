#!/usr/bin/env python3
"""NumPy model of the N-point search pair for B1C at 30.69 MS/s (csrc/bds_acq_pfa31.h), beside tools/proto_pfa32.py and tools/proto_pfa6.py:
N = 613 800 = 31 x 11 x 1800, the row 1800 = 8 x 9 x 25 itself a twiddle-free product.
    python tools/proto_pfa31.py maps      the Good-Thomas maps: 5-D transform == N-point transform, rows in natural k3 order, the rotation of a cell
    python tools/proto_pfa31.py rows      the row pass: CRT positions in the LDS region, the 25 / 9 / 8-point stages, the gather of the lags
    python tools/proto_pfa31.py layout    the inter-pass buffer: tiles of 16 lags, the A-operand rows of a wave item (4 lags x 12 k2 slots)
    python tools/proto_pfa31.py cols      the 11-point stage per lane and the S +- X epilogue of the (re, im) lane pair
    python tools/proto_pfa31.py forward   the forward transform: gather, five dense stages, natural k3 order
    python tools/proto_pfa31.py all
No hi-only bound pass is built (every output block is computed with hi + lo coefficients once), so there is no margin to model."""
import sys

import numpy as np

K1, K2, K3 = 31, 11, 1800
KA, KB, KC = 8, 9, 25
N = K1 * K2 * K3
DIMS = (K1, K2, KA, KB, KC)
TILE, WAVE_LAGS, NB, NI = 16, 4, 4, 2
TILES = (K3 + TILE - 1) // TILE
CELL_ELEMS = TILES * K1 * K2 * TILE * 2
PER_LANE = (K3 + 63) // 64


def lag_of(t1, t2, t3):
    return (t1 * (N // K1) + t2 * (N // K2) + t3 * (N // K3)) % N


def bw_piece(k1, k2, t3):
    """Element index (fp16 complex, 4 bytes) of the 2-element piece (component 0, component 1) of (k1, k2, t3) in its cell."""
    return ((t3 // TILE * K1 + k1) * K2 + k2) * (TILE * 2) + (t3 % TILE) * 2


def pos_of_k3(k3):
    """Position of spectrum index k3 in a row's LDS region [k3 mod 8][k3 mod 9][k3 mod 25]."""
    return ((k3 % KA) * KB + k3 % KB) * KC + k3 % KC


def pos_of_t3(t3):
    """Position of lag part t3 = t8 225 + t9 200 + t25 72 mod 1800 in the region [t8][t9][t25] after the three stages."""
    return ((t3 % KA) * KB + (5 * t3) % KB) * KC + (8 * t3) % KC


def k3_of(i8, i9, i25):
    return (225 * i8 + 1000 * i9 + 576 * i25) % K3


def n_of(n1, n2, n8, n9, n25):
    """Sample index of the gather of the forward transform."""
    return (n1 * (N // K1) + n2 * (N // K2) + n8 * (N // KA) + n9 * (N // KB) + n25 * (N // KC)) % N


# ---- the small transforms of the row pass, step by step as the kernel forms them (inverse: exp(+2 pi j ..)) ------------------------
def dft3(a, b, c):
    h3 = np.sqrt(3.0) / 2
    s, d = b + c, h3 * 1j * (b - c)
    m = a - 0.5 * s
    return a + s, m + d, m - d


def slot9_index(s):
    return s // 3 + 3 * (s % 3)


def dft9_slots(x):
    """x[9] in natural order -> slots; slot s holds output slot9_index(s)."""
    x = list(x)
    for j0 in range(3):
        x[j0], x[j0 + 3], x[j0 + 6] = dft3(x[j0], x[j0 + 3], x[j0 + 6])
    w = np.exp(2j * np.pi * np.arange(9) / 9)
    x[4], x[7], x[5], x[8] = x[4] * w[1], x[7] * w[2], x[5] * w[2], x[8] * w[4]
    for t0 in range(3):
        x[3 * t0], x[3 * t0 + 1], x[3 * t0 + 2] = dft3(x[3 * t0], x[3 * t0 + 1], x[3 * t0 + 2])
    return x


def dft4(a0, a1, a2, a3):
    s02, d02, s13, d13 = a0 + a2, a0 - a2, a1 + a3, 1j * (a1 - a3)
    return [s02 + s13, d02 + d13, s02 - s13, d02 - d13]


def dft8(x):
    """Natural order in and out."""
    r2 = np.sqrt(0.5)
    e, o = dft4(x[0], x[2], x[4], x[6]), dft4(x[1], x[3], x[5], x[7])
    o[1] = r2 * ((o[1].real - o[1].imag) + 1j * (o[1].real + o[1].imag))
    o[2] = 1j * o[2]
    o[3] = r2 * (-(o[3].real + o[3].imag) + 1j * (o[3].real - o[3].imag))
    return [e[t] + o[t] for t in range(4)] + [e[t] - o[t] for t in range(4)]


def slot25_index(s):
    return 5 * (s % 5) + s // 5


def row_pass(prod, swap_maps=False):
    """Rows of one component as k_pfa31_rows walks them: prod[..., k3] (natural order) -> y[..., t3] (natural lag order), the unnormalised
    inverse 1800-point transform.  swap_maps: the deliberate error of tests/test_pfa31_cases.py (lag gather with the spectrum map)."""
    prod = np.asarray(prod, dtype=np.complex128)
    lead = prod.shape[:-1]
    region = np.zeros(lead + (K3,), dtype=np.complex128)
    region[..., pos_of_k3(np.arange(K3))] = prod
    r = region.reshape(lead + (KA, KB, KC))
    r = np.fft.ifft(r, axis=-1) * KC  # pfa::pk_radix25: slot s holds output slot25_index(s) and is written back to that index
    out9 = dft9_slots([r[..., q, :] for q in range(9)])  # [slot][..., i8, i25]
    r9 = np.empty_like(r)
    for s in range(9):
        r9[..., slot9_index(s), :] = out9[s]
    r8 = np.stack(dft8([r9[..., q, :, :] for q in range(8)]), axis=-3)
    region = r8.reshape(lead + (K3,))
    t3 = np.arange(K3)
    return region[..., pos_of_k3(t3) if swap_maps else pos_of_t3(t3)]


# ---- column pass ---------------------------------------------------------------------------------------------------------------------
def wave_rows(t0):
    """The 48 A-operand rows of a wave item at lag t0: rows[g][ai] = (t3, k2) of row ai of MFMA row group g, as k_pfa31_cols loads them:
    lag t0 + (ai >> 2), k2 slot 4 g + (ai & 3); slot 11 reads k2 = 10 again and its output is dropped."""
    rows = np.empty((3, 16, 2), dtype=np.int64)
    for g in range(3):
        for ai in range(16):
            rows[g, ai] = (t0 + (ai >> 2), min(4 * g + (ai & 3), K2 - 1))
    return rows


def lane_outputs(lane):
    """The t2 lane `lane` reports per output block, for t1 = (16 nb + (lane & 15)) >> 1 and the lag t0 + (lane >> 4): even lane
    t2 = 0 .. 5, odd lane 10 .. 6 (its slot 0 is no output)."""
    return [K2 - i for i in range(1, 6)] if lane & 1 else list(range(6))


def coef_matrix():
    """The B operand of the 31-point stage: coef[kappa = 2 k1 + ri_in][o = 2 t1 + ri_out], 64 x 64 (rows / columns past 62 are zeros)."""
    c = np.zeros((32 * NI, 16 * NB))
    k1, t1 = np.meshgrid(np.arange(K1), np.arange(K1), indexing="ij")
    ang = 2 * np.pi * ((k1 * t1) % K1) / K1
    c[0:2 * K1:2, 0:2 * K1:2], c[1:2 * K1:2, 0:2 * K1:2] = np.cos(ang), -np.sin(ang)
    c[0:2 * K1:2, 1:2 * K1:2], c[1:2 * K1:2, 1:2 * K1:2] = np.sin(ang), np.cos(ang)
    return c


def real_dft11(v):
    """F[t] = sum_k v[k] exp(+2 pi j k t / 11), t = 0..5, of a real sequence, as pfa31::real_dft11 forms it: (P[6], Q[6])."""
    c, s = np.cos(2 * np.pi * np.arange(11) / 11), np.sin(2 * np.pi * np.arange(11) / 11)
    e = [0.0] + [v[k] + v[11 - k] for k in range(1, 6)]
    d = [0.0] + [v[k] - v[11 - k] for k in range(1, 6)]
    P, Q = np.empty((6,) + np.shape(v)[1:]), np.zeros((6,) + np.shape(v)[1:])
    P[0] = v[0] + sum(e)
    for t in range(1, 6):
        P[t] = v[0] + sum(e[k] * c[(k * t) % 11] for k in range(1, 6))
        Q[t] = sum(d[k] * s[(k * t) % 11] for k in range(1, 6))
    return P, Q


def pair_epilogue(z, missing_conj=False):
    """|y[t2]|^2, t2 = 0..10, of y = the 11-point inverse transform (unnormalised) of complex z[11], as the lane pair forms it.
    missing_conj: the deliberate error of tests/test_pfa31_cases.py (the odd lane takes the even lane's sign of x)."""
    Pe, Qe = real_dft11(z.real)
    Po, Qo = real_dft11(z.imag)
    out = np.empty((11,) + np.shape(z)[1:])
    out[0] = Pe[0] ** 2 + Po[0] ** 2
    for t in range(1, 6):
        S = Pe[t] ** 2 + Qe[t] ** 2 + Po[t] ** 2 + Qo[t] ** 2
        x = Po[t] * Qe[t] - Qo[t] * Pe[t]  # even lane: x = Q P' - P Q'
        out[t] = S + 2 * x
        out[11 - t] = S + 2 * x if missing_conj else S - 2 * x  # odd lane: x = Q_o P_e - P_o Q_e
    return out


# ---- forward transform -----------------------------------------------------------------------------------------------------------------
def forward(x):
    """Spectrum rows [31][11][1800] in natural k3 order of x[N], as pfa31::forward: gather, five dense stages, store."""
    idx = np.indices(DIMS)
    T = x[n_of(*idx)]
    for ax in range(5):
        T = np.fft.fft(T, axis=ax)
    out = np.empty((K1, K2, K3), dtype=np.complex128)
    out[:, :, k3_of(idx[2][0, 0], idx[3][0, 0], idx[4][0, 0])] = T
    return out


def rotate_rows(X, s, plus=False):
    """The rows of the cell rotated by s: row (k1, k2) reads row ((k1 - s) mod 31, (k2 - s) mod 11) at k3 - s.  plus: the deliberate error."""
    s = -s if plus else s
    return np.roll(X[(np.arange(K1)[:, None] - s) % K1, (np.arange(K2)[None, :] - s) % K2], s, axis=2)


def inter_pass(Xrows, Crows, s, plus=False, swap_maps=False):
    """The inter-pass values [31][11][1800] (k1, k2, lag t3) of one component of the cell rotated by s."""
    return row_pass(rotate_rows(Xrows, s, plus) * Crows, swap_maps)


def column_pass(B, missing_conj=False, last_tile_of=None):
    """|y|^2 over all lags [N] of one component from its inter-pass values, as k_pfa31_cols forms it: the 31-point stage as the real 64 x 64
    matrix product, the 11-point stage per lane with the S +- X epilogue.  last_tile_of: the deliberate error of tests/test_pfa31_cases.py
    (the lags of the short last tile read from that tile instead)."""
    if last_tile_of is not None:
        B = B.copy()
        B[:, :, (TILES - 1) * TILE:] = B[:, :, last_tile_of * TILE:last_tile_of * TILE + K3 - (TILES - 1) * TILE]
    a = np.zeros((32 * NI, K2, K3))
    a[0:2 * K1:2], a[1:2 * K1:2] = B.real, B.imag
    o = np.einsum("kab,ko->oab", a, coef_matrix())
    z = o[0:2 * K1:2] + 1j * o[1:2 * K1:2]  # [t1][k2][t3]
    zr = np.moveaxis(z, 1, 0)               # [k2][t1][t3]
    e = pair_epilogue(zr, missing_conj)     # [t2][t1][t3]
    out = np.empty(N)
    t2, t1, t3 = np.meshgrid(np.arange(K2), np.arange(K1), np.arange(K3), indexing="ij")
    out[lag_of(t1, t2, t3)] = e
    return out


def search_cell(Xrows, Crows, s, **err):
    """|correlation|^2 of one component over all lags [N] through the model of both passes (float64): Xrows = forward(signal),
    Crows = conj(forward(code)) / N."""
    rows_err = {k: v for k, v in err.items() if k in ("plus", "swap_maps")}
    cols_err = {k: v for k, v in err.items() if k in ("missing_conj", "last_tile_of")}
    return column_pass(inter_pass(Xrows, Crows, s, **rows_err), **cols_err)


def maps():
    rng = np.random.default_rng(0)
    k = np.arange(N)
    k_of = np.empty((K1, K2, K3), dtype=np.int64)
    k_of[k % K1, k % K2, k % K3] = k
    lag = lag_of(np.arange(K1)[:, None, None], np.arange(K2)[None, :, None], np.arange(K3)[None, None, :])
    assert np.array_equal(np.sort(k_of.ravel()), k) and np.array_equal(np.sort(lag.ravel()), k)
    t3 = np.arange(K3)
    assert np.array_equal(np.sort(pos_of_k3(t3)), t3) and np.array_equal(np.sort(pos_of_t3(t3)), t3)
    i8, i9, i25 = np.meshgrid(np.arange(KA), np.arange(KB), np.arange(KC), indexing="ij")
    assert np.array_equal(pos_of_k3(k3_of(i8, i9, i25)), (i8 * KB + i9) * KC + i25)
    assert np.array_equal(pos_of_t3((i8 * 225 + i9 * 200 + i25 * 72) % K3), (i8 * KB + i9) * KC + i25)
    Y = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    y3 = np.fft.ifftn(Y[k_of]) * N
    y1 = np.fft.ifft(Y) * N
    err = np.max(np.abs(y3 - y1[lag])) / np.max(np.abs(y1))
    print(f"maps: 3-D transform at lag_of(t1, t2, t3) vs the N-point transform: max error {err:.2e}")
    assert err < 1e-10
    for s in (1, 8, 9, 11, 25, 30, 31, 200, 400, 1799, 1800, 1801):
        assert np.array_equal(np.roll(Y, s)[k_of], rotate_rows(Y[k_of], s))
    print("maps: rotation by s = every coordinate minus s (s = 1 .. 1801): exact")


def rows():
    rng = np.random.default_rng(1)
    p = rng.standard_normal(K3) + 1j * rng.standard_normal(K3)
    ref = np.fft.ifft(p) * K3
    err = np.max(np.abs(row_pass(p) - ref)) / np.max(np.abs(ref))
    print(f"rows: CRT scatter, 25 / 9 / 8-point stages, gather of the lags vs the 1800-point transform: max error {err:.2e}")
    assert err < 1e-12
    x9 = rng.standard_normal(9) + 1j * rng.standard_normal(9)
    got = np.empty(9, dtype=complex)
    got[[slot9_index(s) for s in range(9)]] = dft9_slots(x9)
    assert np.allclose(got, np.fft.ifft(x9) * 9) and np.allclose(dft8(list(x9[:8])), np.fft.ifft(x9[:8]) * 8)
    print(f"rows: {PER_LANE} points per lane, the last one on {K3 - 64 * (PER_LANE - 1)} lanes")


def layout():
    k1, k2, t3 = np.meshgrid(np.arange(K1), np.arange(K2), np.arange(K3), indexing="ij")
    piece = bw_piece(k1, k2, t3).ravel()
    assert len(np.unique(piece)) == N and piece.max() + 2 <= CELL_ELEMS and np.all(piece % 2 == 0)
    print(f"layout: {TILES} tiles of {TILE} lags, {CELL_ELEMS * 4} bytes per cell, a tile = {K1 * K2 * TILE * 8} contiguous bytes; the last tile holds {K3 - (TILES - 1) * TILE} lags")
    seen = set()
    for wave in range(4):
        r = wave_rows(WAVE_LAGS * wave)
        seen |= {tuple(r[g, ai]) for g in range(3) for ai in range(16)}
    assert seen == {(t, k) for t in range(TILE) for k in range(K2)}
    print("layout: the 4 x 48 A-operand rows of a workgroup item are the tile's 16 lags x 11 k2 (k2 = 10 twice)")


def cols():
    rng = np.random.default_rng(2)
    worst = 0.0
    for _ in range(100):
        z = rng.standard_normal(K2) + 1j * rng.standard_normal(K2)
        ref = np.abs(np.fft.ifft(z) * K2) ** 2
        worst = max(worst, np.max(np.abs(pair_epilogue(z) - ref)) / ref.max())
    print(f"cols: S +- X of the lane pair vs |11-point inverse transform|^2: max error {worst:.2e}")
    assert worst < 1e-12
    assert sorted(lane_outputs(0) + lane_outputs(1)) == list(range(K2))
    z = rng.standard_normal(K1) + 1j * rng.standard_normal(K1)
    a = np.zeros(32 * NI)
    a[0:2 * K1:2], a[1:2 * K1:2] = z.real, z.imag
    o = a @ coef_matrix()
    ref = np.fft.ifft(z) * K1
    assert np.allclose(o[0:2 * K1:2] + 1j * o[1:2 * K1:2], ref) and np.all(o[2 * K1:] == 0)
    print("cols: the 64 x 64 real coefficient matrix is the 31-point inverse transform")


def forward_check():
    rng = np.random.default_rng(3)
    x = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    X = np.fft.fft(x)
    k = np.arange(N)
    got = np.empty(N, dtype=complex)
    got[k] = forward(x)[k % K1, k % K2, k % K3]
    err = np.max(np.abs(got - X)) / np.max(np.abs(X))
    print(f"forward: gather + five dense stages + natural k3 order vs the N-point transform: max error {err:.2e}")
    assert err < 1e-10


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    for name, f in (("maps", maps), ("rows", rows), ("layout", layout), ("cols", cols), ("forward", forward_check)):
        if what in (name, "all"):
            f()
