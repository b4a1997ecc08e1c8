#!/usr/bin/env python3
"""NumPy model of the N-point search pair for B2a at 99.375 MS/s (csrc/bds_acq_pfa6.h), beside tools/proto_pfa32.py: N = 198 750 = 53 x 6 x 625.
    python tools/proto_pfa6.py maps      the Good-Thomas maps: 3-D transform == N-point transform, and the rotation of a cell
    python tools/proto_pfa6.py layout    the inter-pass buffer: tiles of 32 lags, the A-operand rows of a wave item (8 lags x 6 k2)
    python tools/proto_pfa6.py cols      the 6-point stage per lane and the S +- X epilogue of the (re, im) lane pair
    python tools/proto_pfa6.py step      the fractional Doppler step: acqStep N / fs = p / q, bin q m + j = spectrum j rotated by p m
    python tools/proto_pfa6.py all
No hi-only bound pass is built (every output block is computed with hi + lo coefficients once), so there is no margin to model."""
import sys
from math import gcd

import numpy as np

K1, K2, K3 = 53, 6, 625
N = K1 * K2 * K3
MP, TILE, WAVE_LAGS, MAX_Q = 27, 32, 8, 5
TILES = (K3 + TILE - 1) // TILE
CELL_ELEMS = TILES * MP * K2 * TILE * 4
FS = 99.375e6


def lag_of(t1, t2, t3):
    return (t1 * (N // K1) + t2 * (N // K2) + t3 * (N // K3)) % N


def bw_piece(mp, k2, t3):
    """Element index (fp16 complex, 4 bytes) of the 4-element piece of (mp, k2, t3) in its cell."""
    return ((t3 // TILE * MP + mp) * K2 + k2) * (TILE * 4) + (t3 % TILE) * 4


def step_ratio(step, fs, n=N):
    """acqStep N / fs = p / q in lowest terms, decided in integers as pfa6::step_ratio does; None when step or fs is no whole number of hertz."""
    if not (1 <= step <= 1e9 and 1 <= fs <= 1e12) or step != int(step) or fs != int(fs):
        return None
    a, b = int(step) * int(n), int(fs)
    g = gcd(a, b)
    return a // g, b // g


def admitted(step, fs, nbins, n=N):
    """(p, q) when the pair takes this step (q <= 5, p >= 1, every rotation below N), else None."""
    r = step_ratio(step, fs, n)
    if r is None or r[1] > MAX_Q or r[0] < 1 or r[0] * ((nbins + r[1] - 1) // r[1]) >= n:
        return None
    return r


def cell_of_bin(b, p, q):
    """0-based bin b = q m + j -> (spectrum index j, rotation p m)."""
    return b % q, (b // q) * p


def carrier(f, n=N, fs=FS):
    """exp(+1i f phasePoints), phasePoints = n 2 pi / fs (B2a/acquisition.m:146, 199), the turn count reduced exactly for whole hertz."""
    k = np.arange(n, dtype=np.int64)
    return np.exp(2j * np.pi * ((int(f) * k) % int(fs)) / fs)


def wave_rows(t0):
    """The 48 A-operand rows of a wave item at lag t0: rows[g][ai] = (t3, k2) of row ai of MFMA row group g, as k_pfa6_cols loads them:
    value i = 4 g + (ai & 3) of the lane quarter ai >> 2 is lag 2 (ai >> 2) + i // 6, k2 = i % 6."""
    rows = np.empty((3, 16, 2), dtype=np.int64)
    for g in range(3):
        for ai in range(16):
            i = 4 * g + (ai & 3)
            rows[g, ai] = (t0 + 2 * (ai >> 2) + i // 6, i % 6)
    return rows


def lane_outputs(lane):
    """What lane `lane` of a wave reports per output block nb: [(u, t2)] with the lag t0 + 2 (lane >> 4) + u, for t1 = (16 nb + (lane & 15)) >> 1:
    the even lane of the (re, im) pair holds t2 = 0, 1, 2, the odd lane 3, 5, 4."""
    odd = lane & 1
    return [(u, (3 if i == 0 else 6 - i) if odd else i) for u in range(2) for i in range(3)]


def real_dft6(a):
    """F[t] = sum_k a[k] exp(+2 pi j k t / 6), t = 0..3, of a real sequence, as pfa::real_dft6 forms it: (re[4], im[4])."""
    h3 = np.sqrt(3.0) / 2
    s0, d0, s1, d1, s2, d2 = a[0] + a[3], a[0] - a[3], a[1] + a[4], a[1] - a[4], a[2] + a[5], a[2] - a[5]
    s12, d12 = s1 + s2, d1 - d2
    return np.array([s0 + s12, d0 + 0.5 * d12, s0 - 0.5 * s12, d0 - d12]), np.array([0.0, h3 * (d1 + d2), h3 * (s1 - s2), 0.0])


def pair_epilogue(z):
    """|y[t2]|^2, t2 = 0..5, of y = the 6-point inverse transform (unnormalised) of complex z[6], as the lane pair forms it: the even lane
    holds A = DFT6(re z), the odd lane B = DFT6(im z); S = |A|^2 + |B|^2 and x = Q P' - P Q' (' = the partner's) give S + 2 x =
    |y[t]|^2 in the even lane and |y[6 - t]|^2 in the odd lane; t = 0 and 3 are their own mirrors."""
    Pe, Qe = real_dft6(z.real)
    Po, Qo = real_dft6(z.imag)
    out = np.empty(6)
    out[0] = Pe[0] ** 2 + Po[0] ** 2  # even lane, slot 0
    out[3] = Pe[3] ** 2 + Po[3] ** 2  # odd lane, slot 0
    for t in (1, 2):
        S = Pe[t] ** 2 + Qe[t] ** 2 + Po[t] ** 2 + Qo[t] ** 2
        out[t] = S + 2 * (Po[t] * Qe[t] - Qo[t] * Pe[t])      # even lane: x = Q P' - P Q'
        out[6 - t] = S + 2 * (Pe[t] * Qo[t] - Qe[t] * Po[t])  # odd lane
    return out


def maps():
    rng = np.random.default_rng(0)
    k = np.arange(N)
    k_of = np.empty((K1, K2, K3), dtype=np.int64)
    k_of[k % K1, k % K2, k % K3] = k
    lag = lag_of(np.arange(K1)[:, None, None], np.arange(K2)[None, :, None], np.arange(K3)[None, None, :])
    assert np.array_equal(np.sort(k_of.ravel()), k) and np.array_equal(np.sort(lag.ravel()), k)
    Y = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    y3 = np.fft.ifftn(Y[k_of]) * N  # inverse 3-D transform of the CRT-ordered spectrum
    y1 = np.fft.ifft(Y) * N
    err = np.max(np.abs(y3 - y1[lag])) / np.max(np.abs(y1))
    print(f"maps: 3-D transform at lag_of(t1, t2, t3) vs the N-point transform: max error {err:.2e}")
    assert err < 1e-10
    for s in (1, 5, 6, 7, 52, 53, 624, 625, 640):  # the rotation of a cell: index k - s <-> every coordinate minus s
        X = np.roll(Y, s)[k_of]
        rot = Y[k_of][(np.arange(K1)[:, None, None] - s) % K1, (np.arange(K2)[None, :, None] - s) % K2, (np.arange(K3)[None, None, :] - s) % K3]
        assert np.array_equal(X, rot)
    print("maps: rotation by s = every coordinate minus s (s = 1 .. 640): exact")


def layout():
    mp, k2, t3 = np.meshgrid(np.arange(MP), np.arange(K2), np.arange(K3), indexing="ij")
    piece = bw_piece(mp, k2, t3).ravel()
    assert len(np.unique(piece)) == MP * K2 * K3 and piece.max() + 4 <= CELL_ELEMS
    print(f"layout: {TILES} tiles of {TILE} lags, {CELL_ELEMS * 4} bytes per cell, a tile = {MP * K2 * TILE * 16} contiguous bytes; the last tile holds {K3 - (TILES - 1) * TILE} lags")
    seen = set()
    for wave in range(4):
        rows = wave_rows(WAVE_LAGS * wave)
        for g in range(3):
            for ai in range(16):
                seen.add(tuple(rows[g, ai]))
    assert seen == {(t, k) for t in range(TILE) for k in range(K2)}
    print("layout: the 4 x 48 A-operand rows of a workgroup item are the tile's 32 lags x 6 k2, each once")


def cols():
    rng = np.random.default_rng(2)
    worst = 0.0
    for _ in range(100):
        z = rng.standard_normal(K2) + 1j * rng.standard_normal(K2)
        ref = np.abs(np.fft.ifft(z) * K2) ** 2
        worst = max(worst, np.max(np.abs(pair_epilogue(z) - ref)) / ref.max())
    print(f"cols: S +- X of the lane pair vs |6-point inverse transform|^2: max error {worst:.2e}")
    assert worst < 1e-12
    t2s = sorted(t2 for lane in (0, 1) for u, t2 in lane_outputs(lane) if u == 0)
    assert t2s == list(range(6))


def step():
    rng = np.random.default_rng(3)
    x = np.round(20 * rng.standard_normal(N))
    f0 = 0 - 5000  # IF - acqSearchBand (B2a/initSettings.m: IF = 0)
    for hz in (400, 250, 500, 1000):
        nbins = int(round(10000 / hz)) + 1
        p, q = admitted(hz, FS, nbins)
        base = [np.fft.fft(carrier(f0 + hz * j) * x) for j in range(q)]
        worst = 0.0
        for b in range(nbins):
            j, s = cell_of_bin(b, p, q)
            X = np.fft.fft(carrier(f0 + hz * b) * x)
            worst = max(worst, np.linalg.norm(X - np.roll(base[j], s)) / np.linalg.norm(X))
        print(f"step: acqStep {hz} Hz = {p}/{q} of a spectrum bin, {nbins} bins from {q} transforms: max error {worst:.2e} of the norm")
        assert worst < 1e-12
    assert admitted(410, FS, 25) is None and step_ratio(410, FS) == (41, 50)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    for name, f in (("maps", maps), ("layout", layout), ("cols", cols), ("step", step)):
        if what in (name, "all"):
            f()
