"""Column pass k_pfa_cols<2, false> of the N-point pair (csrc/bds_acq_pfa.h) at the edges of its K dimension and of its work list,
through the stage driver tools/probe/pfa_stages.hip against the float64 model of tests/pfa_cases.py (the driver, the contract checks
and the tolerances are those of tests/test_pfa_stages_gpu.py).

Value mode (keep = 0: every lag comes back through the values' and the exhaustive pass): buffers that are non-zero only in the rows
k1 = 48..52 -- the last K step of the 53-point stage, most of which is padding --, only in k1 = 52 -- the row that shares its row pair
with the zero row 53 --, and only in k1 = 0..47, the three full K steps.  Tolerance: the column tolerance of the stage tests,
EPS_COLS = 4 x the value of profiles/pfa_stage_errors.txt; the eps each case needs is printed (measured on MI355X: 6.173e-7 / 6.093e-8 /
1.420e-6 -- without a peak in a column no output carries the accumulation error of something much larger than itself).

Sieve mode (keep = 0.996): ncells in {1, 3} x grid in {1, 2, 3, 7} x qchunk in {1, 4}.  196 and 588 items over 1, 2, 3 and 7
workgroups: equal and unequal runs per workgroup, with qchunk = 4 runs that start inside a chunk.  The peaks sit where an index mask can
lose them: t3 = 3120 and 3124 (the last tile holds 5 lags: its second wave has one live lag, its last two waves none) and t1 = 52 (the
last output block holds 5 of 8 t1).  The contract is check_sieve's: cell maxima, every lag within `keep` of the maximum listed, the
running bounds, the wave-item count.
"""
import functools

import numpy as np
import pytest

import pfa_cases as pc
import test_pfa_stages_gpu as st
from test_pfa_stages_gpu import driver  # noqa: F401  (the module-scoped fixture: builds the stage driver, or takes BDS_PFA_STAGES_EXE)

pytestmark = pytest.mark.gpu

K1_RANGES = {"k1_48_52": (48, 53), "k1_52": (52, 53), "k1_0_47": (0, 48)}


@functools.lru_cache(maxsize=None)
def cell_k1_range(name):
    lo, hi = K1_RANGES[name]
    z = pc.noise_floor(np.random.default_rng(200 + lo), 1.0)
    z[:, :lo] = 0.0
    z[:, hi:] = 0.0
    return pc.ColsCell(name, pc.round_h2(z))


@pytest.mark.parametrize("name", list(K1_RANGES))
def test_cols_value_mode_k1_range(driver, tmp_path, name):  # noqa: F811
    cell = cell_k1_range(name)
    launch = pc.Launch(1, 0, 1, 1, pc.host_grid(1, 1), pc.NP, True, 0.0)
    (r,) = st.split_launches(driver.run(pc.cols_case([cell], [launch]), tmp_path, timeout=90), [launch])
    assert pc.guard_intact(r.head_guard) and pc.guard_intact(r.tail_guard)
    assert r.count == pc.NP and len(r.entries) == r.count
    assert r.stats[0] == r.stats[1] == r.stats[2] == pc.WAVE_ITEMS_PER_CELL and r.stats[3] == 7 * r.stats[0]
    assert np.all(r.entries["cell"] == 0) and np.array_equal(np.sort(r.entries["lag"]), np.arange(pc.NP))  # each lag exactly once
    _, inv = pc.lag_grid()
    got = np.empty(pc.NP)
    got[inv[r.entries["lag"]]] = r.entries["v"]
    st.report(f"cols value mode [{name}] eps", cell.measure_eps(got))
    err, tol = np.abs(got - cell.a.reshape(-1)), cell.value_tolerance(st.EPS_COLS)
    assert np.all(err <= tol), (name, int(np.argmax(err / tol)), float(np.max(err / tol)))
    high = cell.a.reshape(-1) >= 0.5 * cell.max
    st.report(f"cols value mode [{name}], lags at or above half the maximum: worst |error| / maximum", float(np.max(err[high])) / cell.max)
    assert np.all(err[high] <= st.BUDGET * cell.max)
    lag = int(r.cellmax_lag[0])
    tol = np.minimum(tol, st.BUDGET * cell.max)
    assert abs(float(r.cellmax_v[0]) - cell.max) <= tol[int(np.argmax(cell.a))] and cell.a.reshape(-1)[inv[lag]] >= cell.max - tol[inv[lag]]


# (t1, t2, t3, fraction of the cell's peak value): every listed peak is above keep = 0.996 of the maximum, none within 2e-5 of it
EDGE_PEAKS = (
    ((52, 5, 3124, 1.0), (52, 7, 3120, 0.9985), (17, 0, 3124, 0.999), (3, 6, 3120, 0.998), (52, 11, 100, 0.9975), (0, 0, 3121, 0.9992)),
    ((52, 6, 3120, 1.0), (52, 0, 3124, 0.9995), (51, 9, 3119, 0.9988)),
    ((30, 4, 3124, 1.0), (52, 2, 17, 0.9981), (8, 8, 3120, 0.9993), (52, 10, 3124, 0.9979)),
)
EDGE_LEVEL = (2000.0, 1500.0, 1750.0)
SIEVE_CELL0, SIEVE_LB_DIV = 1, 2  # run-wide cells 1 | 2 3: the second and third cell share a running bound


@functools.lru_cache(maxsize=None)
def cell_edge_peaks(i):
    rng = np.random.default_rng(210 + i)
    y = pc.noise_floor(rng, 1.0)
    for t1, t2, t3, f in EDGE_PEAKS[i]:
        pc.plant(y, rng, t1, t2, t3, EDGE_LEVEL[i] * f)
    return pc.ColsCell(f"edge_peaks{i}", pc.spectrum_of(y), claims=len(EDGE_PEAKS[i]))


def sieve_launches():
    return [pc.Launch(n, SIEVE_CELL0, SIEVE_LB_DIV, q, g, 1 << 16, True, pc.KEEP) for n in (1, 3) for g in (1, 2, 3, 7) for q in (1, 4)]


def test_cols_sieve_edges_small_grids(driver, tmp_path):  # noqa: F811
    cells = [cell_edge_peaks(i) for i in range(3)]
    lag_grid, _ = pc.lag_grid()
    launches = sieve_launches()
    assert len(launches) == 16
    results = st.split_launches(driver.run(pc.cols_case(cells, launches), tmp_path, timeout=90), launches)
    for launch, r in zip(launches, results):
        try:
            st.check_sieve(r, cells, launch)
            # the planted peaks by name: those at or above the threshold of their cell's bound group
            gm = pc.group_maxima(cells[:launch.ncells], launch.cell0, launch.lb_div)
            for i in range(launch.ncells):
                listed = set(r.entries["lag"][r.entries["cell"] == launch.cell0 + i].tolist())
                for t1, t2, t3, _ in EDGE_PEAKS[i]:
                    if cells[i].a[t1, t2, t3] >= pc.KEEP * (1.0 + pc.BAND) * gm[i]:
                        assert int(lag_grid[t1, t2, t3]) in listed, (i, t1, t2, t3)
                assert int(r.cellmax_lag[launch.cell0 + i]) == int(lag_grid[EDGE_PEAKS[i][0][:3]])
        except AssertionError as e:
            raise AssertionError(f"{launch}: {e}") from e
