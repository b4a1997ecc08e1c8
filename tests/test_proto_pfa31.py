"""tools/proto_pfa31.py, the NumPy model of the opt-in N-point search pair for B1C at 30.69 MS/s (csrc/bds_acq_pfa31.h): its five parts run,
and its pieces -- the index maps of the 1800-point row, the small transforms, the row mapping of a wave item, the lanes' outputs, the
11-point S +- X epilogue -- are what the kernel's comments say they are."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import proto_pfa31 as pp  # noqa: E402


@pytest.mark.parametrize("part", ["maps", "rows", "layout", "cols", "forward"])
def test_the_model_runs(part, capsys):
    getattr(pp, "forward_check" if part == "forward" else part)()
    assert part in capsys.readouterr().out


def test_sizes():
    assert pp.N == 613800 == 8 * 9 * 25 * 11 * 31 == int(round(30.69e6 * 20e-3)) and pp.K3 == pp.KA * pp.KB * pp.KC
    for i, a in enumerate(pp.DIMS):
        for b in pp.DIMS[i + 1:]:
            assert np.gcd(a, b) == 1
    assert pp.TILES == 113 and pp.CELL_ELEMS * 4 == 4932224 and pp.K1 * pp.K2 * pp.TILE * 8 == 43648
    assert pp.K1 * pp.K2 * 2 * pp.K3 * 4 < 2 ** 24  # the signal spectrum with doubled rows inside the buffer-load offset range
    assert 2 * pp.K1 <= 32 * pp.NI and 2 * pp.K1 <= 16 * pp.NB and pp.PER_LANE == 29


def test_row_maps():
    k3 = np.arange(pp.K3)
    i8, i9, i25 = k3 % 8, k3 % 9, k3 % 25
    assert np.array_equal(pp.k3_of(i8, i9, i25), k3)
    # the Good-Thomas pair inside the row: exp(2 pi j k3 t3 / 1800) = exp(2 pi j (i8 t8 / 8 + i9 t9 / 9 + i25 t25 / 25))
    rng = np.random.default_rng(5)
    t3 = rng.integers(pp.K3, size=200)
    k = rng.integers(pp.K3, size=200)
    p = pp.pos_of_t3(t3)
    t8, t9, t25 = p // 225, p // 25 % 9, p % 25
    assert np.array_equal((t8 * 225 + t9 * 200 + t25 * 72) % pp.K3, t3)
    lhs = (k * t3) % pp.K3 / pp.K3
    rhs = (k % 8 * t8 % 8) / 8 + (k % 9 * t9 % 9) / 9 + (k % 25 * t25 % 25) / 25
    assert np.allclose(np.exp(2j * np.pi * lhs), np.exp(2j * np.pi * rhs), atol=1e-9)
    # half of N later (the second code period of the 20 ms) is t3 + 900
    assert pp.lag_of(7, 4, 1000) == (pp.lag_of(7, 4, 100) + pp.N // 2) % pp.N


def test_small_transforms():
    rng = np.random.default_rng(6)
    for n, f in ((9, None), (8, pp.dft8)):
        x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        if n == 9:
            got = np.empty(9, dtype=complex)
            got[[pp.slot9_index(s) for s in range(9)]] = pp.dft9_slots(x)
        else:
            got = np.array(f(list(x)))
        assert np.allclose(got, np.fft.ifft(x) * n, atol=1e-13)
    assert sorted(pp.slot25_index(s) for s in range(25)) == list(range(25)) and sorted(pp.slot9_index(s) for s in range(9)) == list(range(9))
    p = rng.standard_normal((3, 2, pp.K3)) + 1j * rng.standard_normal((3, 2, pp.K3))
    assert np.allclose(pp.row_pass(p), np.fft.ifft(p, axis=-1) * pp.K3, atol=1e-10)
    assert not np.allclose(pp.row_pass(p, swap_maps=True), np.fft.ifft(p, axis=-1) * pp.K3, atol=1e-3)


def test_wave_rows_and_lane_outputs():
    for t0 in (0, 4, 1796):
        rows = pp.wave_rows(t0)
        assert set(map(tuple, rows.reshape(-1, 2))) == {(t0 + u, k) for u in range(4) for k in range(11)}
        # the accumulators of lane quarter ks: rows 4 ks .. 4 ks + 3 of the three groups = the 11 k2 of lag ks, then k2 = 10 again
        for ks in range(4):
            vals = [tuple(rows[g, 4 * ks + rr]) for g in range(3) for rr in range(4)]
            assert vals == [(t0 + ks, min(k, 10)) for k in range(12)]
    for lane in (0, 16, 34, 62):
        assert sorted(pp.lane_outputs(lane) + pp.lane_outputs(lane + 1)) == list(range(11))
    assert pp.lane_outputs(0) == [0, 1, 2, 3, 4, 5] and pp.lane_outputs(1) == [10, 9, 8, 7, 6]


def test_real_dft11_and_the_pair_epilogue():
    rng = np.random.default_rng(9)
    for _ in range(20):
        a = rng.standard_normal(11)
        P, Q = pp.real_dft11(a)
        F = np.fft.ifft(a) * 11
        assert np.allclose(P, F[:6].real, atol=1e-13) and np.allclose(Q, F[:6].imag, atol=1e-13)
        z = rng.standard_normal(11) + 1j * rng.standard_normal(11)
        assert np.allclose(pp.pair_epilogue(z), np.abs(np.fft.ifft(z) * 11) ** 2, rtol=1e-12, atol=1e-12)
        assert not np.allclose(pp.pair_epilogue(z, missing_conj=True), np.abs(np.fft.ifft(z) * 11) ** 2, rtol=1e-3)
    # a single line: the outputs of a mirror pair differ by the full 2 X
    z = np.zeros(11, dtype=complex)
    z[1] = 2 - 1j
    assert np.allclose(pp.pair_epilogue(z), 5.0)
