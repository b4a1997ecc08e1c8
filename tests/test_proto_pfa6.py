"""tools/proto_pfa6.py, the NumPy model of the opt-in N-point search pair for B2a at 99.375 MS/s (csrc/bds_acq_pfa6.h): its four parts run,
and its pieces -- the row mapping of a wave item, the lanes' outputs, the 6-point S +- X epilogue, the step rule -- are what the kernel's
comments say they are."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import proto_pfa6 as pp  # noqa: E402


@pytest.mark.parametrize("part", ["maps", "layout", "cols", "step"])
def test_the_model_runs(part, capsys):
    getattr(pp, part)()
    assert part in capsys.readouterr().out


def test_sizes():
    assert pp.N == 198750 == 53 * 6 * 625 and pp.TILES == 20 and pp.CELL_ELEMS * 4 == 1658880
    assert pp.MP * pp.K2 * pp.TILE * 16 == 82944  # a column workgroup's item: the block size of bds_acq_pfa.h (27 x 12 x 16 x 16)
    assert 5 * 53 * 6 * 1250 * 4 < 2 ** 24     # five signal spectra with doubled rows inside the buffer-load offset range


def test_wave_rows_and_lane_outputs():
    for t0 in (0, 8, 616):
        rows = pp.wave_rows(t0)
        assert sorted(map(tuple, rows.reshape(-1, 2))) == [(t0 + u, k) for u in range(8) for k in range(6)]
        # the accumulators of lane quarter ks: rows 4 ks .. 4 ks + 3 of the three groups = the 6 k2 of lag 2 ks, then of lag 2 ks + 1
        for ks in range(4):
            vals = [tuple(rows[g, 4 * ks + rr]) for g in range(3) for rr in range(4)]
            assert vals == [(t0 + 2 * ks + u, k) for u in range(2) for k in range(6)]
    # the (re, im) lane pair covers t2 = 0..5 once per lag
    for lane in (0, 16, 34, 62):
        both = pp.lane_outputs(lane) + pp.lane_outputs(lane + 1)
        assert sorted(both) == [(u, t2) for u in range(2) for t2 in range(6)]
    assert [t2 for _, t2 in pp.lane_outputs(0)[:3]] == [0, 1, 2] and [t2 for _, t2 in pp.lane_outputs(1)[:3]] == [3, 5, 4]


def test_real_dft6_and_the_pair_epilogue():
    rng = np.random.default_rng(9)
    for _ in range(20):
        a = rng.standard_normal(6)
        re, im = pp.real_dft6(a)
        F = np.fft.ifft(a) * 6
        assert np.allclose(re, F[:4].real, atol=1e-13) and np.allclose(im, F[:4].imag, atol=1e-13)
        z = rng.standard_normal(6) + 1j * rng.standard_normal(6)
        assert np.allclose(pp.pair_epilogue(z), np.abs(np.fft.ifft(z) * 6) ** 2, rtol=1e-12, atol=1e-12)
    # a single line: the outputs of a mirror pair differ by the full 2 X
    z = np.zeros(6, dtype=complex)
    z[1] = 2 - 1j
    assert np.allclose(pp.pair_epilogue(z), 5.0)


def test_step_rule():
    fs = 99.375e6
    assert pp.step_ratio(400, fs) == (4, 5) and pp.step_ratio(250, fs) == (1, 2) and pp.step_ratio(500, fs) == (1, 1) and pp.step_ratio(1000, fs) == (2, 1)
    assert pp.step_ratio(410, fs) == (41, 50) and pp.admitted(410, fs, 25) is None
    assert pp.step_ratio(400.5, fs) is None and pp.admitted(400.5, fs, 26) is None
    assert pp.admitted(400, fs, 26) == (4, 5) and pp.admitted(400, fs, 5 * 49688) is None  # 4 x 49 688 >= N
    assert [pp.cell_of_bin(b, 4, 5) for b in (0, 4, 5, 25)] == [(0, 0), (4, 0), (0, 4), (0, 20)]
