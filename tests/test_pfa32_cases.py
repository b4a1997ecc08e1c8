"""The cases of tests/pfa32_cases.py are what tests/test_pfa32_stages_gpu.py takes them for -- checked on the CPU, before a GPU sees
them: the CRT / lag maps are bijections on N = 1 060 000, the tile map covers every (mp, k2, t3) once, no lag of a column case sits in
the ambiguity band of a threshold it is judged against, the lane-sharing pairs share a lane, the tie ties, and the FFT-based references
agree with direct sums in natural order."""
import numpy as np
import pytest

import pfa32_cases as pc

SIEVE_CELLS = (pc.cell_noise, pc.cell_near, pc.cell_tie)


def test_index_maps_are_bijections_and_good_thomas():
    assert pc.NP == 1060000 == 53 * 32 * 625 and np.gcd(53, 32) == np.gcd(53, 625) == np.gcd(32, 625) == 1
    k_of = pc.crt_index()
    assert np.array_equal(np.sort(k_of.ravel()), np.arange(pc.NP))
    lag, inv = pc.lag_grid()
    assert np.array_equal(np.sort(lag.ravel()), np.arange(pc.NP)) and np.array_equal(lag.ravel()[inv], np.arange(pc.NP))
    # the Good-Thomas pair: exp(2 pi j k t / N) = exp(2 pi j (k1 t1 / 53 + k2 t2 / 32 + k3 t3 / 625))
    rng = np.random.default_rng(1)
    k = rng.integers(pc.NP, size=50)
    t1, t2, t3 = rng.integers(pc.K1, size=50), rng.integers(pc.K2, size=50), rng.integers(pc.K3, size=50)
    t = pc.lag_of(t1, t2, t3)
    lhs = (k * t) % pc.NP / pc.NP
    rhs = ((k % pc.K1) * t1 % pc.K1) / pc.K1 + ((k % pc.K2) * t2 % pc.K2) / pc.K2 + ((k % pc.K3) * t3 % pc.K3) / pc.K3
    assert np.allclose(np.exp(2j * np.pi * lhs), np.exp(2j * np.pi * rhs), atol=1e-9)
    # the rotation of a Doppler bin: spectrum index k - s <-> ((k1 - s) mod 53, (k2 - s) mod 32, (k3 - s) mod 625), s past 625 included
    for s in (1, 33, 53, 625, 640, 1252):
        kk = (k - s) % pc.NP
        assert np.array_equal(k_of[(k % pc.K1 - s) % pc.K1, (k % pc.K2 - s) % pc.K2, (k % pc.K3 - s) % pc.K3], kk)


def test_tile_map_covers_every_piece_once():
    mp, k2, t3 = np.meshgrid(np.arange(pc.MP), np.arange(pc.K2), np.arange(pc.K3), indexing="ij")
    piece = pc.bw_piece(mp, k2, t3).ravel()
    assert np.all(piece % 4 == 0) and piece.min() == 0 and piece.max() + 4 <= pc.CELL_ELEMS
    assert len(np.unique(piece)) == pc.MP * pc.K2 * pc.K3
    assert pc.TILES == 79 and pc.CELL_ELEMS == 79 * 27 * 32 * 8 * 4
    # a column workgroup's item -- the 8 lags of a tile, all (mp, k2) -- is one contiguous block
    for tile in (0, 40, 77):
        blk = np.sort(pc.bw_piece(mp[:, :, :8], k2[:, :, :8], 8 * tile + t3[:, :, :8]).ravel())
        assert blk[0] == tile * pc.MP * pc.K2 * 32 and np.array_equal(np.diff(blk), np.full(len(blk) - 1, 4))
    # bw_pack's transposition against bw_piece, pad row and pad lags included
    z = np.arange(2 * pc.K1 * pc.K2 * pc.K3, dtype=np.float64).reshape(2, pc.K1, pc.K2, pc.K3) % 2039
    words = pc.bw_pack(z + 0j)
    assert words.size == pc.CELL_ELEMS
    for c, k1, k2_, t3_ in ((0, 0, 0, 0), (1, 52, 31, 624), (0, 17, 15, 7), (1, 18, 16, 8), (0, 51, 3, 623), (1, 1, 1, 616)):
        assert pc.unpack_h2(words[pc.bw_piece(k1 // 2, k2_, t3_) + 2 * c + (k1 & 1)]) == z[c, k1, k2_, t3_]
    assert np.all(words[pc.bw_piece(26, np.arange(32)[:, None], np.arange(pc.K3)[None, :]) + np.array([1, 3])[:, None, None]] == 0)
    assert np.all(words[pc.bw_piece(5, 7, 625):pc.bw_piece(5, 7, 625) + 28] == 0xFFFFFFFF)  # the 7 pad lags of the last tile
    full = pc.bw_unpack_words(words)
    assert np.array_equal(full[:, :pc.K1, :, :pc.K3], pc.pack_h2(z + 0j))


def test_a_lane_holds_eight_t2_and_the_lanes_cover_the_32():
    """t2 = e + 2 tai + 16 h + 4 tbi over (e, h) x (tai, tbi): every t2 once, and lane_of groups exactly those eight"""
    seen = {}
    for e in range(2):
        for h in range(2):
            t2s = [e + 2 * tai + 16 * h + 4 * tbi for tai in range(2) for tbi in range(4)]
            assert len({pc.lane_of((0, t, 0)) for t in t2s}) == 1
            seen[(e, h)] = t2s
    assert sorted(sum(seen.values(), [])) == list(range(32))


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
            assert items in grids and any(items % g for g in grids)
            smaller += any(g < q * n for g in grids)
            larger += any(g > q * n for g in grids)
    assert smaller and larger
    assert pc.items_of(1, 8) > pc.TILES  # the last chunk of 8 runs past tile 78


def test_near_threshold_cell():
    cell = pc.cell_near()
    a = cell.a
    thr = pc.KEEP * cell.max
    both = 0
    for p, q, above in cell.notes["pairs"]:
        assert pc.shares_lane(p, q) and p != q
        assert p[2] == q[2] and p[0] % 8 == q[0] % 8 and p[1] % 2 == q[1] % 2 and (p[1] < 16) == (q[1] < 16)
        assert a[p] >= thr * (1 + pc.BAND)
        assert (a[q] >= thr * (1 + pc.BAND)) == above and (above or a[q] < thr * (1 - pc.BAND))
        both += above
    assert both >= 8 and any(p[2] == 623 for p, _, _ in cell.notes["pairs"])
    last = a[:, :, pc.K3 - 1]
    assert np.count_nonzero(last >= thr * (1 + pc.BAND)) == 1  # one listed lag in the wave of t3 = 624 (its second lag is masked)
    assert np.count_nonzero(a >= 0.98 * cell.max) == pc.NEAR_LOW + pc.NEAR_HIGH
    assert np.count_nonzero(a >= thr) == pc.NEAR_HIGH


def test_tie_cell():
    cell = pc.cell_tie()
    v = cell.a[:, :, pc.TIE_T3]
    assert v.size == 1696 and np.ptp(v) <= 1e-12 * v.max()
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
    assert n == cell.notes["peaks"] == 120
    # both sides of every boundary of the layout: the wave's two lags, two waves of a workgroup, two tiles, the single-lag last tile
    t3s = set(pc.EDGE_T3)
    assert {0, 1} <= t3s and {1, 2} <= t3s and {7, 8} <= t3s and {615, 616} <= t3s and {623, 624} <= t3s
    assert 7 // pc.TILE != 8 // pc.TILE and 623 // pc.TILE != 624 // pc.TILE and 1 // pc.WAVE_LAGS != 2 // pc.WAVE_LAGS


def test_fft_references_against_direct_sums():
    """sampled outputs to 1e-10 of the rms: the forward transform, the row pass, the column pass and the pair end to end"""
    rng = np.random.default_rng(5)
    n = 0
    x, ref = pc.forward_input(), pc.forward_reference()
    rms = np.sqrt(np.mean(np.abs(ref) ** 2))
    for k in [0, pc.NP - 1] + list(rng.integers(pc.NP, size=8)):
        b = int(k) & 1
        d = pc.direct_npoint(x[b], k, -1) * pc.FWD_SCALE
        assert abs(d - ref[b, k % pc.K1, k % pc.K2, k % pc.K3]) < 1e-10 * rms
        n += 1
    for s, slot in ((53, 1), (640, 0)):
        ref = pc.rows_reference(s, slot)
        rms = np.sqrt(np.mean(np.abs(ref) ** 2))
        for _ in range(45):
            c, k1, k2, t3 = int(rng.integers(2)), int(rng.integers(pc.K1)), int(rng.integers(pc.K2)), int(rng.integers(pc.K3))
            assert abs(pc.direct_row(s, slot, c, k1, k2, t3) - ref[c, k1, k2, t3]) < 1e-10 * rms
            n += 1
    for cell in (pc.cell_near(), pc.cell_edges()):
        rms = np.sqrt(np.mean(cell.m))
        picks = [(0, 0, 0), (52, 31, 624)] + [(int(rng.integers(pc.K1)), int(rng.integers(pc.K2)), int(rng.integers(pc.K3))) for _ in range(43)]
        for t1, t2, t3 in picks:
            c = int(rng.integers(2))
            d = pc.direct_col(cell.words, c, t1, t2, t3)
            assert abs(abs(d) ** 2 - cell.m[c, t1, t2, t3]) < 1e-10 * rms * max(rms, abs(d))
            n += 1
    a = pc.e2e_reference(657, 1)
    Y = pc.product_spectrum(657, 1)
    rms = np.sqrt(np.mean(a ** 2))
    for _ in range(10):
        t = int(rng.integers(pc.NP))
        d = pc.W0 * abs(pc.direct_npoint(Y[0], t, +1)) + pc.W1 * abs(pc.direct_npoint(Y[1], t, +1))
        assert abs(d - a[t]) < 1e-10 * rms
        n += 1
    assert n == 200
