"""The cases of tests/pfa6_cases.py are what tests/test_pfa6_stages_gpu.py takes them for -- checked on the CPU, before a GPU sees them:
the CRT / lag maps are bijections on N = 198 750, the tile map covers every (mp, k2, t3) once and a tile is one contiguous block, no lag
of a column case sits in the ambiguity band of a threshold it is judged against, the lane-sharing pairs share a lane, the tie ties, the
masked ranges have their edges where they claim, the FFT-based references agree with direct sums in natural order -- and the fractional
Doppler step: fft(carr_b x) is the rotated fft(carr_(b mod q) x) for every bin of the grid at 400, 250, 500 and 1000 Hz, 410 Hz is
refused, and the public header declares the switch."""
import os
import re

import numpy as np
import pytest

import pfa6_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIEVE_CELLS = (pc.cell_noise, pc.cell_near, pc.cell_tie)


def test_index_maps_are_bijections_and_good_thomas():
    assert pc.NP == 198750 == 53 * 6 * 625 and np.gcd(53, 6) == np.gcd(53, 625) == np.gcd(6, 625) == 1
    k_of = pc.crt_index()
    assert np.array_equal(np.sort(k_of.ravel()), np.arange(pc.NP))
    lag, inv = pc.lag_grid()
    assert np.array_equal(np.sort(lag.ravel()), np.arange(pc.NP)) and np.array_equal(lag.ravel()[inv], np.arange(pc.NP))
    # the Good-Thomas pair: exp(2 pi j k t / N) = exp(2 pi j (k1 t1 / 53 + k2 t2 / 6 + k3 t3 / 625))
    rng = np.random.default_rng(1)
    k = rng.integers(pc.NP, size=50)
    t1, t2, t3 = rng.integers(pc.K1, size=50), rng.integers(pc.K2, size=50), rng.integers(pc.K3, size=50)
    t = pc.lag_of(t1, t2, t3)
    lhs = (k * t) % pc.NP / pc.NP
    rhs = ((k % pc.K1) * t1 % pc.K1) / pc.K1 + ((k % pc.K2) * t2 % pc.K2) / pc.K2 + ((k % pc.K3) * t3 % pc.K3) / pc.K3
    assert np.allclose(np.exp(2j * np.pi * lhs), np.exp(2j * np.pi * rhs), atol=1e-9)
    # the rotation of a cell: spectrum index k - s <-> ((k1 - s) mod 53, (k2 - s) mod 6, (k3 - s) mod 625), s past 625 included
    for s in (1, 5, 6, 7, 52, 53, 624, 625, 640):
        kk = (k - s) % pc.NP
        assert np.array_equal(k_of[(k % pc.K1 - s) % pc.K1, (k % pc.K2 - s) % pc.K2, (k % pc.K3 - s) % pc.K3], kk)
    # half of N later (the second code period of the 2 ms) is t2 + 3
    assert pc.lag_of(7, 4, 100) == (pc.lag_of(7, 1, 100) + pc.NP // 2) % pc.NP


def test_tile_map_covers_every_piece_once():
    mp, k2, t3 = np.meshgrid(np.arange(pc.MP), np.arange(pc.K2), np.arange(pc.K3), indexing="ij")
    piece = pc.bw_piece(mp, k2, t3).ravel()
    assert np.all(piece % 4 == 0) and piece.min() == 0 and piece.max() + 4 <= pc.CELL_ELEMS
    assert len(np.unique(piece)) == pc.MP * pc.K2 * pc.K3
    assert pc.TILES == 20 and pc.CELL_ELEMS == 20 * 27 * 6 * 32 * 4 and pc.WAVE_ITEMS_PER_CELL == 79
    # a column workgroup's item -- the 32 lags of a tile, all (mp, k2) -- is one contiguous block of 82 944 bytes
    for tile in (0, 10, 18):
        blk = np.sort(pc.bw_piece(mp[:, :, :32], k2[:, :, :32], 32 * tile + t3[:, :, :32]).ravel())
        assert blk[0] == tile * pc.MP * pc.K2 * 128 and np.array_equal(np.diff(blk), np.full(len(blk) - 1, 4)) and len(blk) * 16 == 82944
    # the last tile: 17 lags, inside the tile's block
    last = pc.bw_piece(mp[:, :, :17], k2[:, :, :17], 608 + t3[:, :, :17]).ravel()
    assert last.min() == 19 * pc.MP * pc.K2 * 128 and last.max() + 4 <= pc.CELL_ELEMS and 625 - 19 * 32 == 17
    # bw_pack's transposition against bw_piece, pad row and pad lags included
    z = np.arange(2 * pc.K1 * pc.K2 * pc.K3, dtype=np.float64).reshape(2, pc.K1, pc.K2, pc.K3) % 2039
    words = pc.bw_pack(z + 0j)
    assert words.size == pc.CELL_ELEMS
    for c, k1, k2_, t3_ in ((0, 0, 0, 0), (1, 52, 5, 624), (0, 17, 3, 31), (1, 18, 2, 32), (0, 51, 3, 607), (1, 1, 1, 608)):
        assert pc.unpack_h2(words[pc.bw_piece(k1 // 2, k2_, t3_) + 2 * c + (k1 & 1)]) == z[c, k1, k2_, t3_]
    assert np.all(words[pc.bw_piece(26, np.arange(6)[:, None], np.arange(pc.K3)[None, :]) + np.array([1, 3])[:, None, None]] == 0)
    assert np.all(words[pc.bw_piece(5, 4, 625):pc.bw_piece(5, 4, 625) + 60] == 0xFFFFFFFF)  # the 15 pad lags of the last tile
    full = pc.bw_unpack_words(words)
    assert np.array_equal(full[:, :pc.K1, :, :pc.K3], pc.pack_h2(z + 0j))


@pytest.mark.parametrize("step", [400, 250, 500, 1000])
def test_fractional_step_identity(step):
    """B2a/acquisition.m:190-201 in float64: for every bin b = q m + j of the grid, fft(carr_b x) equals fft(carr_j x) rotated by p m, to
    1e-12 of its norm"""
    fs, band, IF = 99.375e6, 5000, 13.55e6
    nbins = int(round(2 * band / step)) + 1
    p, q = pc.admitted(step, fs, nbins)
    assert (p, q) == {400: (4, 5), 250: (1, 2), 500: (1, 1), 1000: (2, 1)}[step]
    rng = np.random.default_rng(step)
    x = np.round(20 * rng.standard_normal(pc.NP))
    f0 = IF - band
    base = [np.fft.fft(pc.carrier(f0 + step * j) * x) for j in range(q)]
    for b in range(nbins):
        j, s = pc.cell_of_bin(b, p, q)
        assert j == b % q and s == p * (b // q) and s < pc.NP
        X = np.fft.fft(pc.carrier(f0 + step * b) * x)
        assert np.linalg.norm(X - np.roll(base[j], s)) <= 1e-12 * np.linalg.norm(X), (step, b)


def test_admission_rule():
    fs = 99.375e6
    assert pc.step_ratio(410, fs) == (41, 50) and pc.admitted(410, fs, 25) is None
    assert pc.admitted(400, fs, 26) == (4, 5) and pc.admitted(250, fs, 41) == (1, 2) and pc.admitted(500, fs, 21) == (1, 1) and pc.admitted(1000, fs, 11) == (2, 1)
    assert pc.admitted(399.5, fs, 26) is None and pc.admitted(400, 99.375e6 + 0.5, 26) is None  # not whole hertz: no exact ratio
    assert pc.admitted(100, fs, 101) == (1, 5) and pc.admitted(50, fs, 201) is None             # q = 10
    assert pc.admitted(400, 62e6, 26) is None                                                   # another rate: 400 N / fs = 159 / 124 of this N
    assert pc.admitted(1000, fs, 2 * pc.NP) is None                                             # a rotation past N


def test_header_declares_the_switch():
    h = open(os.path.join(ROOT, "include", "bds_mi355x.h")).read()
    assert re.search(r"BDS_API\s+int\s+bds_acq_set_b2a_npoint\s*\(\s*bds_ctx\s*\*\s*ctx\s*,\s*int\s+on\s*\)\s*;", h)
    assert "acquisition.m:187-211" in h
    from bds_amd import native

    assert "bds_acq_set_b2a_npoint" in native.EXPORTS and hasattr(native.Context, "acq_set_b2a_npoint")
    import inspect

    import bds_amd

    assert "b2a_npoint" in inspect.signature(bds_amd.acquisition).parameters


def test_rows_runs_cover_the_rotations_and_spectra():
    seen_rot, seen_spec, seen_p = set(), set(), set()
    for run in pc.ROWS_RUNS:
        assert len(run.bins) == len(run.slots)
        for b in run.bins:
            spec, s = pc.cell_of_bin(b, run.p, run.q)
            assert spec < pc.NSPEC
            seen_rot.add(s), seen_spec.add(spec), seen_p.add(run.p)
        assert run.gc == 1 or len(run.bins) % run.gc  # chunks of one, or a short last chunk
    assert {0, 1, 5, 6, 7, 52, 53, 624, 625, 640} <= seen_rot and {0, 1, 4} <= seen_spec and seen_p == {1, 4}


@pytest.mark.parametrize("build", SIEVE_CELLS + (pc.cell_edges,), ids=lambda f: f.__name__)
def test_single_cell_thresholds_are_unambiguous(build):
    cell = build()
    req, band = pc.required_and_band(cell, cell.max)
    assert band == 0
    assert len(req) >= max(1, cell.claims)


def test_multi_cell_thresholds_are_unambiguous():
    cells = [f() for f in pc.MULTI_CELLS]
    for n in pc.MULTI_NCELLS:
        gm = pc.group_maxima(cells[:n], pc.MULTI_CELL0, pc.MULTI_LB_DIV)
        for cell, g in zip(cells[:n], gm):
            assert pc.required_and_band(cell, g)[1] == 0, (n, cell.name)
    gm = pc.group_maxima(cells, pc.MULTI_CELL0, pc.MULTI_LB_DIV)
    assert gm[0] == cells[0].max and gm[1] == gm[2] == max(cells[1].max, cells[2].max) and gm[3] == cells[3].max
    smaller = larger = 0
    for n in pc.MULTI_NCELLS:
        for q in pc.MULTI_QCHUNK:
            grids = pc.multi_grids(n, q)
            items = pc.items_of(n, q)
            assert items in grids
            smaller += any(g < q * n for g in grids)
            larger += any(g > q * n for g in grids)
    assert smaller and larger
    assert pc.items_of(1, 8) > pc.TILES  # the last chunk of 8 runs past tile 19


def test_near_threshold_cell():
    cell = pc.cell_near()
    a = cell.a
    thr = pc.KEEP * cell.max
    both = 0
    for p, q, above in cell.notes["pairs"]:
        assert pc.shares_lane(p, q) and p != q
        assert p[2] // 2 == q[2] // 2 and p[0] % 8 == q[0] % 8 and (p[1] < 3) == (q[1] < 3)
        assert a[p] >= thr * (1 + pc.BAND)
        assert (a[q] >= thr * (1 + pc.BAND)) == above and (above or a[q] < thr * (1 - pc.BAND))
        both += above
    assert both >= 8 and any(p[2] == 623 for p, _, _ in cell.notes["pairs"])
    last = a[:, :, pc.K3 - 1]
    assert np.count_nonzero(last >= thr * (1 + pc.BAND)) == 1  # one listed lag in the wave of t3 = 624 (its other seven lags are masked)
    assert np.count_nonzero(a >= 0.98 * cell.max) == pc.NEAR_LOW + pc.NEAR_HIGH
    assert np.count_nonzero(a >= thr) == pc.NEAR_HIGH


def test_tie_cell():
    cell = pc.cell_tie()
    v = cell.a[:, :, pc.TIE_T3]
    assert v.size == 318 and np.ptp(v) <= 1e-12 * v.max()
    rest = np.delete(cell.a, pc.TIE_T3, axis=2)
    assert rest.max() < 0.5 * v.min()
    assert abs(v.max() - (pc.W0 + pc.W1) * abs(pc.TIE_VALUE)) < 1e-12


def test_edge_cell_has_a_peak_on_every_edge():
    cell = pc.cell_edges()
    floor = np.median(cell.a)
    n = 0
    for t1 in pc.EDGE_T1:
        for t2 in pc.EDGE_T2:
            for t3 in pc.EDGE_T3:
                assert cell.a[t1, t2, t3] > 100 * floor
                n += 1
    assert n == cell.notes["peaks"] == 96
    # both sides of every boundary of the layout: a lane's two lags, a wave's 8 lags, two tiles, the last full tile, lag 624; the wave of
    # the last tile with one live lag (t0 = 624) and the one with none (t0 = 632 >= 625)
    t3s = set(pc.EDGE_T3)
    assert {0, 1} <= t3s and {7, 8} <= t3s and {31, 32} <= t3s and {607, 608} <= t3s and {623, 624} <= t3s
    assert 7 // pc.WAVE_LAGS != 8 // pc.WAVE_LAGS and 31 // pc.TILE != 32 // pc.TILE and 607 // pc.TILE != 608 // pc.TILE
    assert 608 + 2 * pc.WAVE_LAGS == 624 and 608 + 3 * pc.WAVE_LAGS >= pc.K3


def test_masked_ranges():
    cell = pc.cell_masked()
    L = sorted(cell.notes["lags"])
    assert len(set(L)) == 6 and all(L[i + 1] - L[i] > 2 for i in range(5)) and L[0] > 1
    lag, inv = pc.lag_grid()
    floor = np.median(cell.a)
    for l in L:
        assert cell.a.reshape(-1)[inv[l]] > 100 * floor
    r = pc.mask_ranges()
    m0, m1, m2, m3 = (pc.in_ranges(x) for x in r)
    assert m0[inv[L[0]]] and m0[inv[L[1]]] and not m0[inv[L[2]]] and not m0[inv[L[3]]] and m0[inv[L[2] + 1]] and m0[inv[L[3] - 1]]
    assert not m0[inv[L[0] - 1]] and not m0[inv[L[1] + 1]]
    assert m1[inv[L[4]]] and m1[inv[L[5]]] and not m1[inv[L[1]]] and not m1[inv[L[2]]] and L[5] + 1 < pc.NP and not m1[inv[L[5] + 1]]
    assert m2.sum() == 1 and m2[inv[L[3]]] and m3.sum() == 0
    assert m0.sum() == (L[1] - L[0] + 1) + (L[3] - L[2] - 1)
    # the thresholds of the masked sieve launches are unambiguous (judged on the buffer cell each entry reads: 1, 1, 0, 1)
    for rng4, c in zip(r[:3], (cell, cell, pc.cell_noise())):
        allowed = pc.in_ranges(rng4)
        top = np.where(allowed, c.a.reshape(-1), -1.0).max()
        assert pc.required_and_band(c, top, pc.KEEP, allowed)[1] == 0


def test_fft_references_against_direct_sums():
    """sampled outputs to 1e-10 of the rms: the forward transform, the row pass, the column pass and the pair end to end"""
    rng = np.random.default_rng(5)
    n = 0
    x, ref = pc.forward_input(), pc.forward_reference()
    rms = np.sqrt(np.mean(np.abs(ref) ** 2))
    for k in [0, pc.NP - 1] + list(rng.integers(pc.NP, size=8)):
        b = int(k) % pc.FWD_BATCH
        d = pc.direct_npoint(x[b], k, -1) * pc.FWD_SCALE
        assert abs(d - ref[b, k % pc.K1, k % pc.K2, k % pc.K3]) < 1e-10 * rms
        n += 1
    for spec, s, slot in ((0, 53, 1), (4, 640, 0)):
        ref = pc.rows_reference(spec, s, slot)
        rms = np.sqrt(np.mean(np.abs(ref) ** 2))
        for _ in range(45):
            c, k1, k2, t3 = int(rng.integers(2)), int(rng.integers(pc.K1)), int(rng.integers(pc.K2)), int(rng.integers(pc.K3))
            assert abs(pc.direct_row(spec, s, slot, c, k1, k2, t3) - ref[c, k1, k2, t3]) < 1e-10 * rms
            n += 1
    for cell in (pc.cell_near(), pc.cell_edges()):
        rms = np.sqrt(np.mean(cell.m))
        picks = [(0, 0, 0), (52, 5, 624)] + [(int(rng.integers(pc.K1)), int(rng.integers(pc.K2)), int(rng.integers(pc.K3))) for _ in range(43)]
        for t1, t2, t3 in picks:
            c = int(rng.integers(2))
            d = pc.direct_col(cell.words, c, t1, t2, t3)
            assert abs(abs(d) ** 2 - cell.m[c, t1, t2, t3]) < 1e-10 * rms * max(rms, abs(d))
            n += 1
    a = pc.e2e_reference(1, 656, 1)
    Y = pc.product_spectrum(1, 656, 1)
    rms = np.sqrt(np.mean(a ** 2))
    for _ in range(10):
        t = int(rng.integers(pc.NP))
        d = pc.W0 * abs(pc.direct_npoint(Y[0], t, +1)) + pc.W1 * abs(pc.direct_npoint(Y[1], t, +1))
        assert abs(d - a[t]) < 1e-10 * rms
        n += 1
    assert n == 200
