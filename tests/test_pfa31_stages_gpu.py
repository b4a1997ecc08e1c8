"""Every output of every stage of the opt-in N-point search pair for B1C at 30.69 MS/s (csrc/bds_acq_pfa31.h) against float64: the forward
transforms, the row pass k_pfa31_rows, the column pass k_pfa31_cols in value mode (keep = 0: every lag comes back through the exhaustive
listing) and in sieve mode (the protocol as a contract), and the pair end to end.  tools/probe/pfa31_stages.hip launches the stages exactly
as csrc/bds_acq.hip does and does no arithmetic of its own; inputs and references are tests/pfa31_cases.py's, whose model
tests/test_pfa31_cases.py ties to the direct correlation and the oracle on the CPU.

Every driver run is a child process under its own time limit.  A run that ends by signal, by time limit or with a HIP error marks the
module: every later test fails at once without starting another GPU process.  Nothing is retried.

Tolerances, all against the float64 reference, in the forms of tests/test_pfa6_stages_gpu.py (measured values:
profiles/pfa31_stage_errors.txt; each test prints what it measures):
  column pass   fp32 arithmetic.  Per lag sum_c w_c (sqrt(m_c + EPS S_c) - sqrt(m_c)) + 1e-6 a (pfa31_cases.ColsCell.value_tolerance),
                EPS = 4 x the smallest value that passes every value-mode lag.  Lags at or above half the cell's maximum and every value
                the sieve reports are held to 1e-5 of the maximum.
  row pass, forward transforms   fp16 storage.  Per real component 2^-11 |ref| + 2^-25 + C x (row's largest |ref|), C = 4 x the smallest
                value that passes, and C <= 1e-5.
  end to end    1e-3 of the maximum per lag: the bound the suite asserts for fp16 storage.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pfa31_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BUDGET = 1e-5
# 4 x the measured values of profiles/pfa31_stage_errors.txt (MI355X)
C_FWD = 4 * 1.954e-7   # measured 1.954e-7 (the signal shape and the code shape)
C_ROWS = 4 * 1.138e-7  # measured 1.138e-7 (the run across a PRN boundary), 8.911e-8, 8.690e-8, 9.187e-8
assert max(C_ROWS, C_FWD) <= BUDGET
# measured 8.798e-6 on the two value-mode cells (2.111e-7 on the noise cell alone): a floor-level output in the column (lag t3) of a peak
# hundreds of times the floor carries the fp32 error of the whole column (341 outputs), which the S of its mirror pair does not measure
# (the finding of tests/test_pfa_stages_gpu.py).  What a sieve decision can turn on is held to the budget itself: every lag at or above
# half the cell's maximum (measured 1.492e-7 of the maximum) and every value the sieve reports.
EPS_COLS = 4 * 8.798e-6
E2E_TOL = 1e-3         # measured worst 1.774e-4 of the maximum


def report(name, value):
    print(f"\npfa31_stage_errors: {name} = {value:.3e}")


class Driver:
    def __init__(self, exe):
        self.exe = exe
        self.broken = None

    def run(self, arrays, tmp_path, timeout=60):
        """One child process: case file in, result arrays out."""
        if self.broken:
            pytest.fail("no further GPU process after: " + self.broken)
        case, out = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
        pc.write_arrays(case, arrays)
        try:
            r = subprocess.run([self.exe, case, out], capture_output=True, text=True, timeout=timeout)
        except subprocess.TimeoutExpired:
            self.broken = f"the driver ran into its time limit of {timeout} s"
            pytest.fail(self.broken)
        finally:
            os.remove(case)
        if r.returncode == 3:  # the driver refused the case before any launch
            pytest.fail("malformed case: " + r.stderr)
        if r.returncode != 0 or "ok" not in r.stdout:
            self.broken = f"driver exit status {r.returncode}: {r.stderr.strip()[-400:]}"
            pytest.fail(self.broken)
        res = pc.read_arrays(out)
        os.remove(out)
        return res


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = os.environ.get("BDS_PFA31_STAGES_EXE")  # a prebuilt driver, e.g. one built against a modified header to see that the tests bite
    if not exe:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        if not os.path.exists(hipcc):
            pytest.skip("no hipcc on this box")
        exe = str(tmp_path_factory.mktemp("pfa31_stages") / "pfa31_stages")
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-fno-slp-vectorize",
               "-I" + os.path.join(ROOT, "bds-3-b1c-b2a-sdr-receiver_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
               os.path.join(ROOT, "tools", "probe", "pfa31_stages.hip"), "-o", exe]
        subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    return Driver(exe)


# ---- forward transforms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb, doubled, conj, stride", [(1, 1, 0, 2 * pc.NP), (2, 0, 1, pc.NP)], ids=["signal", "codes"])
def test_forward(driver, tmp_path, nb, doubled, conj, stride):
    (dst,) = driver.run(pc.forward_case(nb, doubled, conj, stride), tmp_path)
    dst = dst.view(np.uint32)
    assert not np.any(dst == 0xFFFFFFFF)  # every element written
    if doubled:
        rows = dst.reshape(nb, pc.K1, pc.K2, 2, pc.K3)
        assert np.array_equal(rows[:, :, :, 0], rows[:, :, :, 1])  # the two copies of a row: bit-equal
        got = pc.unpack_h2(rows[:, :, :, 0])
    else:
        got = pc.unpack_h2(dst.reshape(nb, pc.K1, pc.K2, pc.K3))
    ref = pc.forward_reference()[:nb]
    if conj:
        ref = np.conj(ref)
    report(f"forward[{'signal' if doubled else 'codes'}] c", pc.measure_c(got, ref))
    tr, ti = pc.storage_tolerance(ref, C_FWD)
    assert np.all(np.abs(got.real - ref.real) <= tr) and np.all(np.abs(got.imag - ref.imag) <= ti)


# ---- row pass -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", pc.ROWS_RUNS, ids=lambda r: r.name)
def test_rows(driver, tmp_path, run):
    (buf,) = driver.run(pc.rows_case(run), tmp_path)
    buf = buf.view(np.uint32)
    n, g = len(run.bins), pc.ROWS_GUARD
    assert buf.size == n * pc.CELL_ELEMS + 2 * g
    assert pc.guard_intact(buf[:g]) and pc.guard_intact(buf[-g:])
    worst, bad_at = 0.0, []
    for i in range(n):
        w = pc.bw_unpack_words(buf[g + i * pc.CELL_ELEMS:g + (i + 1) * pc.CELL_ELEMS])
        assert np.all(w[:, :, :, pc.K3:] == 0xFFFFFFFF)  # the pad lags of the last tile: never written
        body = w[:, :, :, :pc.K3]
        assert not np.any(body == 0xFFFFFFFF)  # every element of the cell written, the first and the last row included
        got = pc.unpack_h2(body)
        ref = pc.rows_reference(run.bins[i] * run.shift, run.slots[i])
        worst = max(worst, pc.measure_c(got, ref))
        tr, ti = pc.storage_tolerance(ref, C_ROWS)
        bad = (np.abs(got.real - ref.real) > tr) | (np.abs(got.imag - ref.imag) > ti)
        if np.any(bad):
            bad_at.append((i, run.bins[i], np.argwhere(bad)[:5].tolist()))
    report(f"rows[{run.name}] c", worst)
    assert not bad_at, bad_at


# ---- column pass ----------------------------------------------------------------------------------------------------------------
def split_launches(res, launches):
    assert len(res) == 5 * len(launches)
    return [pc.parse_cols(res[5 * i:5 * i + 5]) for i in range(len(launches))]


def sieve_tolerance(cell, pos):
    """What a value the sieve reports may differ by: the per-lag tolerance, and never more than the budget of the cell's maximum."""
    return np.minimum(cell.value_tolerance(EPS_COLS, pos), BUDGET * cell.max)


def check_entries(r, cells, launch, positions_out=None):
    """Every entry of the list: a cell of the launch, a lag of the cell at most once, the reference's value at that lag."""
    _, inv = pc.lag_grid()
    e = r.entries
    local = e["cell"].astype(np.int64) - launch.cell0
    assert np.all((local >= 0) & (local < launch.ncells))
    assert np.all((e["lag"] >= 0) & (e["lag"] < pc.NP))
    for i in range(launch.ncells):
        cell = cells[i]
        sel = e[local == i]
        pos = inv[sel["lag"]]
        assert len(np.unique(pos)) == len(pos), (cell.name, "a lag is listed twice")
        err = np.abs(sel["v"].astype(np.float64) - cell.a.reshape(-1)[pos])
        tol = sieve_tolerance(cell, pos)
        assert np.all(err <= tol), (cell.name, float(np.max(err / tol)))
        if positions_out is not None:
            positions_out.append(pos)


def check_sieve(r, cells, launch):
    """The protocol of the sieve as a contract (bds_acq_sieve.h)."""
    _, inv = pc.lag_grid()
    n = launch.ncells
    cells = cells[:n]
    assert pc.guard_intact(r.head_guard) and pc.guard_intact(r.tail_guard)
    assert r.stats[0] == pc.WAVE_ITEMS_PER_CELL * n
    assert 0 < r.count <= launch.extra_cap and len(r.entries) == r.count
    listed = []
    check_entries(r, cells, launch, listed)
    assert not np.any(r.cellmax_v[:launch.cell0])  # the slots of other launches' cells: untouched
    groups = {}
    for i, cell in enumerate(cells):
        groups.setdefault((launch.cell0 + i) // launch.lb_div, []).append(i)
    for i, cell in enumerate(cells):
        a = cell.a.reshape(-1)
        top = int(np.argmax(a))
        # cellmax: the reference maximum's value, at a lag whose reference value is within the tolerance of it
        v, lag = float(r.cellmax_v[launch.cell0 + i]), int(r.cellmax_lag[launch.cell0 + i])
        assert 0 <= lag < pc.NP
        pos = inv[lag]
        assert abs(v - cell.max) <= sieve_tolerance(cell, np.array([top]))[0], (cell.name, v, cell.max)
        assert a[pos] >= cell.max - sieve_tolerance(cell, np.array([pos]))[0], (cell.name, lag)
        # the list: every lag at or above keep (1 + band) x the largest maximum among the cells sharing the bound
        gmax = max(cells[j].max for j in groups[(launch.cell0 + i) // launch.lb_div])
        req, band = pc.required(cell, gmax, launch.keep)
        assert band == 0
        missing = np.setdiff1d(req, listed[i])
        assert not len(missing), (cell.name, len(missing), "required lags are not listed, e.g. grid position", int(missing[0]))
    # the running bound of a group ends as the largest of its cells' maxima
    for s, members in groups.items():
        assert r.lb[s] == max(r.cellmax_v[[launch.cell0 + j for j in members]])


def test_cols_value_mode(driver, tmp_path):
    """keep = 0 with the bounds zeroed: the list holds each of the N lags of each cell exactly once, ex.v the sieve value -- lag_of, t2_of,
    the t1 >= 31 mask and the odd lane's empty slot, the hi + lo coefficients, the row mapping of the three MFMA row groups with the
    repeated twelfth slot, the 11-point stage and the S +- X epilogue, at every output; on a noise cell and on a cell with one peak 300
    times the floor."""
    cells = [pc.cell_noise(), pc.cell_peak()]
    launch = pc.Launch(2, 0, 1, 1, pc.host_grid(2, 1), 2 * pc.NP, True, 0.0)
    (r,) = split_launches(driver.run(pc.cols_case(cells, [launch]), tmp_path, timeout=90), [launch])
    assert pc.guard_intact(r.head_guard) and pc.guard_intact(r.tail_guard)
    assert r.count == 2 * pc.NP and len(r.entries) == r.count
    assert r.stats[0] == 2 * pc.WAVE_ITEMS_PER_CELL and r.stats[1] == pc.NBLOCKS * r.stats[0]  # every output block of every wave item listed
    _, inv = pc.lag_grid()
    eps = upper = 0.0
    failures = []
    for i, cell in enumerate(cells):
        sel = r.entries[r.entries["cell"] == i]
        assert len(sel) == pc.NP and np.array_equal(np.sort(sel["lag"]), np.arange(pc.NP))  # each lag exactly once
        got = np.empty(pc.NP)
        got[inv[sel["lag"]]] = sel["v"]
        eps = max(eps, cell.measure_eps(got))
        err, tol = np.abs(got - cell.a.reshape(-1)), cell.value_tolerance(EPS_COLS)
        high = cell.a.reshape(-1) >= 0.5 * cell.max
        upper = max(upper, float(np.max(err[high])) / cell.max)
        report(f"cols value mode eps after cell {cell.name}", eps)
        report(f"cols value mode, lags at or above half the maximum: worst |error| / maximum after cell {cell.name}", upper)
        if not np.all(err <= tol):
            failures.append((cell.name, int(np.argmax(err / tol)), float(np.max(err / tol))))
        # the lags a sieve decision can turn on -- the upper half of the cell's values -- to the budget of the maximum
        if not np.all(err[high] <= BUDGET * cell.max):
            failures.append((cell.name, "upper half", upper))
        lag = int(r.cellmax_lag[i])
        tol = np.minimum(tol, BUDGET * cell.max)
        assert abs(float(r.cellmax_v[i]) - cell.max) <= tol[int(np.argmax(cell.a))] and cell.a.reshape(-1)[inv[lag]] >= cell.max - tol[inv[lag]]
    assert not failures, failures


@pytest.mark.parametrize("name", ["peak", "edges"])
def test_cols_sieve_single_cell(driver, tmp_path, name):
    """keep = 0.996 as shipped.  A grid of 7 walks the tiles nearly in order (the threshold of a cell is set before its later tiles are
    judged against it); the host's own grid has every tile of the cell in flight at once."""
    cell = {"peak": pc.cell_peak, "edges": pc.cell_edges}[name]()
    launches = [pc.Launch(1, 0, 1, q, g, 1 << 16, True, pc.KEEP) for q, g in ((1, 7), (1, pc.host_grid(1, 1)), (4, pc.host_grid(1, 4)))]
    results = split_launches(driver.run(pc.cols_case([cell], launches), tmp_path), launches)
    lag_grid = pc.lag_grid()[0]
    for launch, r in zip(launches, results):
        check_sieve(r, [cell], launch)
        if name == "edges":  # the eight peaks above the threshold are all listed (the one at two thirds may be: a wave that met it
            # before the bound had risen lists it, a redundant entry the protocol allows)
            listed = set(r.entries["lag"].tolist())
            for t in ((0, 0, 0), (30, 10, 1799), (15, 5, 15), (1, 6, 16), (29, 4, 1791), (7, 1, 1792), (20, 9, 3), (11, 2, 4)):
                assert int(lag_grid[t]) in listed, t
            assert int(r.cellmax_lag[0]) == int(lag_grid[0, 0, 0])


def test_cols_sieve_multi_cell(driver, tmp_path):
    """ncells x qchunk x grid, cell0 = 3, two cells per running bound: the work list walked in its three digits."""
    cells = [pc.cell_edges(), pc.cell_noise(), pc.cell_peak()]
    launches = [pc.Launch(n, 3, 2, q, g, 1 << 17, True, pc.KEEP) for n in (2, 3) for q in (1, 4) for g in (7, pc.host_grid(n, q))]
    results = split_launches(driver.run(pc.cols_case(cells, launches), tmp_path, timeout=90), launches)
    for launch, r in zip(launches, results):
        try:
            check_sieve(r, cells, launch)
        except AssertionError as e:
            raise AssertionError(f"{launch}: {e}") from e


def test_cols_list_overflow(driver, tmp_path):
    """A list shorter than the qualifying lags (a noise cell with keep = 0.5): the counter runs past the capacity, the slots hold valid
    entries, nothing behind them."""
    cell = pc.cell_noise()
    cap, keep = 100, 0.5
    claims = len(pc.required(cell, cell.max, keep)[0])
    assert claims > cap
    launch = pc.Launch(1, 0, 1, 1, pc.host_grid(1, 1), cap, True, keep)
    (r,) = split_launches(driver.run(pc.cols_case([cell], [launch]), tmp_path), [launch])
    assert r.count >= claims > cap and len(r.entries) == cap
    assert pc.guard_intact(r.head_guard) and pc.guard_intact(r.tail_guard)
    assert np.all(r.entries["v"] > 0)  # every slot taken (the list is prefilled with zeros)
    check_entries(r, [cell], launch)


# ---- the pair ---------------------------------------------------------------------------------------------------------------------
def test_pair_end_to_end(driver, tmp_path):
    """Rows, then columns in value mode on the device's own buffer, against the float64 model of the natural-order spectra at every lag:
    the index maps, the rotation (bin 1999 at one spectrum bin per step: past 1800, and 1999 mod 31, mod 11 and mod 1800 all differ) and
    the fp16 storage together."""
    run = pc.RowsRun("pair", (1999,), (1,), 1, 1)
    assert len({1999 % 31, 1999 % 11, 1999 % 1800, 1999}) == 4
    launch = pc.Launch(1, 0, 1, 1, pc.host_grid(1, 1), pc.NP, True, 0.0)
    res = driver.run(pc.rows_case(run, [launch], write_bw=False), tmp_path, timeout=90)
    assert pc.guard_intact(res[0])
    (r,) = split_launches(res[1:], [launch])
    assert r.count == pc.NP and np.array_equal(np.sort(r.entries["lag"]), np.arange(pc.NP))
    got = np.empty(pc.NP)
    got[r.entries["lag"]] = r.entries["v"]
    ref = pc.e2e_reference(1999, 1)
    worst = float(np.max(np.abs(got - ref)) / ref.max())
    report("pair end to end, worst |error| / maximum", worst)
    assert worst <= E2E_TOL
    assert int(r.cellmax_lag[0]) == int(np.argmax(ref)) or ref[int(r.cellmax_lag[0])] >= ref.max() * (1 - E2E_TOL)
