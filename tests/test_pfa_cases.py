"""The cases of tests/pfa_cases.py are what tests/test_pfa_stages_gpu.py takes them for -- checked on the CPU, before a GPU sees
them: no lag of a column case sits in the ambiguity band of a threshold it is judged against, the lane-sharing pairs share a lane, the
tie ties, the adversarial output would be lost without the bound pass's margin, and the FFT-based references agree with direct sums."""
import numpy as np
import pytest

import pfa_cases as pc

SIEVE_CELLS = (pc.cell_noise, pc.cell_near, pc.cell_tie, pc.cell_adversarial)


def test_index_maps_and_buffer_layout():
    k_of = pc.crt_index()
    assert np.array_equal(np.sort(k_of.ravel()), np.arange(pc.NP))
    lag, inv = pc.lag_grid()
    assert np.array_equal(np.sort(lag.ravel()), np.arange(pc.NP)) and np.array_equal(lag.ravel()[inv], np.arange(pc.NP))
    # the Good-Thomas pair: exp(2 pi j k t / N) = exp(2 pi j (k1 t1 / 53 + k2 t2 / 12 + k3 t3 / 3125))
    rng = np.random.default_rng(1)
    k = rng.integers(pc.NP, size=50)
    t1, t2, t3 = rng.integers(pc.K1, size=50), rng.integers(pc.K2, size=50), rng.integers(pc.K3, size=50)
    t = pc.lag_of(t1, t2, t3)
    lhs = (k * t) % pc.NP / pc.NP
    rhs = ((k % pc.K1) * t1 % pc.K1) / pc.K1 + ((k % pc.K2) * t2 % pc.K2) / pc.K2 + ((k % pc.K3) * t3 % pc.K3) / pc.K3
    assert np.allclose(np.exp(2j * np.pi * lhs), np.exp(2j * np.pi * rhs), atol=1e-9)
    # bw_pack's transposition against bw_piece, pad row and pad lags included
    z = np.arange(2 * pc.K1 * pc.K2 * pc.K3, dtype=np.float64).reshape(2, pc.K1, pc.K2, pc.K3) % 2039
    words = pc.bw_pack(z + 0j)
    assert words.size == pc.CELL_ELEMS
    for c, k1, k2, t3 in ((0, 0, 0, 0), (1, 52, 11, 3124), (0, 17, 5, 15), (1, 18, 6, 16), (0, 51, 3, 3119), (1, 1, 1, 3120)):
        assert pc.unpack_h2(words[pc.bw_piece(k1 // 2, k2, t3) + 2 * c + (k1 & 1)]) == z[c, k1, k2, t3]
    assert np.all(words[pc.bw_piece(26, np.arange(12)[:, None], np.arange(pc.K3)[None, :]) + np.array([1, 3])[:, None, None]] == 0)
    assert np.all(words[pc.bw_piece(5, 7, 3125):pc.bw_piece(5, 7, 3125) + 44] == 0xFFFFFFFF)
    full = pc.bw_unpack_words(words)
    assert np.array_equal(full[:, :pc.K1, :, :pc.K3], pc.pack_h2(z + 0j))


@pytest.mark.parametrize("build", SIEVE_CELLS + (pc.cell_peaks, pc.cell_edges), ids=lambda f: f.__name__)
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
    # the grouping is what the comment beside MULTI_CELLS says: `noise` is judged by `tie`'s maximum, `adversarial` by `peaks`'
    gm = pc.group_maxima(cells, pc.MULTI_CELL0, pc.MULTI_LB_DIV)
    assert gm[0] == cells[0].max and gm[1] == gm[2] == cells[2].max and gm[3] == gm[4] == max(cells[3].max, cells[4].max)
    smaller = larger = 0
    for n in pc.MULTI_NCELLS:
        for q in pc.MULTI_QCHUNK:
            grids = pc.multi_grids(n, q)
            items = pc.items_of(n, q)
            assert items in grids and any(items % g for g in grids)
            smaller += any(g < q * n for g in grids)
            larger += any(g > q * n for g in grids)
    assert smaller and larger  # grids smaller and larger than qchunk x ncells
    assert pc.items_of(1, 8) > pc.TILES  # the last chunk of 8 runs past tile 195


def test_near_threshold_cell():
    cell = pc.cell_near()
    a = cell.a
    thr = pc.KEEP * cell.max
    both = 0
    for p, q, above in cell.notes["pairs"]:
        assert pc.shares_lane(p, q) and p != q
        assert p[2] == q[2] and p[0] % 8 == q[0] % 8 and (p[1] in range(6)) == (q[1] in range(6))
        assert a[p] >= thr * (1 + pc.BAND)
        assert (a[q] >= thr * (1 + pc.BAND)) == above and (above or a[q] < thr * (1 - pc.BAND))
        both += above
    assert both >= 8 and any(p[2] >= 3120 for p, _, _ in cell.notes["pairs"])
    last = a[:, :, pc.K3 - 1]
    assert np.count_nonzero(last >= thr * (1 + pc.BAND)) == 1  # one listed lag in the wave of t3 = 3124 .. 3127
    planted = np.count_nonzero(a >= 0.98 * cell.max)
    assert planted == pc.NEAR_LOW + pc.NEAR_HIGH
    assert np.count_nonzero(a >= thr) == pc.NEAR_HIGH  # a few hundred peaks around the threshold, this many above it


def test_tie_cell():
    cell = pc.cell_tie()
    v = cell.a[:, :, pc.TIE_T3]
    assert v.size == 636 and np.ptp(v) <= 1e-12 * v.max()
    rest = np.delete(cell.a, pc.TIE_T3, axis=2)
    assert rest.max() < 0.5 * v.min()  # the global maximum, far above the floor
    assert abs(v.max() - (pc.W0 + pc.W1) * abs(pc.TIE_VALUE)) < 1e-12


def test_adversarial_cell():
    cell = pc.cell_adversarial()
    t1, t2, t3 = cell.notes["target"]
    lim = pc.KEEP * cell.max
    assert lim * (1 + pc.BAND) <= cell.a[t1, t2, t3] < lim * (1 + 2e-4)
    # the peak that sets the threshold sits in an earlier tile
    p = pc.ADV_PEAK
    assert cell.a[p[0], p[1], p[2]] == cell.max and p[2] // pc.TILE < t3 // pc.TILE
    # without its margin the bound pass -- (largest hi-only sqrt(|y_d|^2 + |y_p|^2))^2 (w0^2 + w1^2) 1.00001 < limit^2 -- skips the wave
    ub = pc.hi_only_bound(cell.notes["z_wave"])
    assert ub * ub * pc.WSUM2 * 1.00001 < (lim * (1 - 5e-5)) ** 2
    # and the inputs are what the docstring says: the lo parts of the target's coefficients all add up
    ch, sh, cl, sl = pc.coef_parts(t1)
    assert cell.notes["gain"] > 2e-4 and np.all(np.abs(cl) <= 2.0 ** -12) and np.all(np.abs(sl) <= 2.0 ** -12)


def test_edge_cell_has_a_peak_on_every_edge():
    cell = pc.cell_edges()
    floor = np.median(cell.a)
    n = 0
    for t1 in pc.EDGE_T1:
        for t2 in pc.EDGE_T2:
            for t3 in pc.EDGE_T3:
                assert cell.a[t1, t2, t3] > 100 * floor
                n += 1
    assert n == cell.notes["peaks"] == 60


def test_fft_references_against_direct_sums():
    """200 sampled outputs, to 1e-10 of the rms: 10 of the forward transform, 90 of the row pass, 90 of the column pass, 10 end to end
    (an N-point direct sum costs 0.1 s, a row's or a column's next to nothing)."""
    rng = np.random.default_rng(5)
    k_of = pc.crt_index()
    lag, inv = pc.lag_grid()
    n = 0
    # forward
    x, ref = pc.forward_input(), pc.forward_reference()
    rms = np.sqrt(np.mean(np.abs(ref) ** 2))
    for k in [0, pc.NP - 1] + list(rng.integers(pc.NP, size=8)):
        b = int(k) & 1
        d = pc.direct_npoint(x[b], k, -1) * pc.FWD_SCALE
        assert abs(d - ref[b, k % pc.K1, k % pc.K2, k % pc.K3]) < 1e-10 * rms
        n += 1
    # row pass: a rotated cell of each slot
    for s, slot in ((53, 1), (400, 0)):
        ref = pc.rows_reference(s, slot)
        rms = np.sqrt(np.mean(np.abs(ref) ** 2))
        for _ in range(45):
            c, k1, k2, t3 = int(rng.integers(2)), int(rng.integers(pc.K1)), int(rng.integers(pc.K2)), int(rng.integers(pc.K3))
            assert abs(pc.direct_row(s, slot, c, k1, k2, t3) - ref[c, k1, k2, t3]) < 1e-10 * rms
            n += 1
    # column pass: from the packed cell through bw_piece
    for cell in (pc.cell_near(), pc.cell_edges()):
        rms = np.sqrt(np.mean(cell.m))
        picks = [(0, 0, 0), (52, 11, 3124)] + [(int(rng.integers(pc.K1)), int(rng.integers(pc.K2)), int(rng.integers(pc.K3))) for _ in range(43)]
        for t1, t2, t3 in picks:
            c = int(rng.integers(2))
            d = pc.direct_col(cell.words, c, t1, t2, t3)
            assert abs(abs(d) ** 2 - cell.m[c, t1, t2, t3]) < 1e-10 * rms * max(rms, abs(d))
            n += 1
    # end to end: the natural-order sum at the lag lag_of names
    a = pc.e2e_reference(57, 1)
    Y = pc.product_spectrum(57, 1)
    rms = np.sqrt(np.mean(a ** 2))
    for _ in range(10):
        t = int(rng.integers(pc.NP))
        d = pc.W0 * abs(pc.direct_npoint(Y[0], t, +1)) + pc.W1 * abs(pc.direct_npoint(Y[1], t, +1))
        assert abs(d - a[t]) < 1e-10 * rms
        n += 1
    assert n == 200
