"""Every output of every stage of the opt-in N-point search pair for B2a at 99.375 MS/s (csrc/bds_acq_pfa6.h) against float64: the forward
transforms, the row pass k_pfa6_rows, the column pass k_pfa6_cols in value mode (keep = 0: every lag comes back through the exhaustive
listing), in sieve mode (the protocol as a contract) and in masked mode (lag ranges and source cells: the second-peak pass), and the pair
end to end.  tools/probe/pfa6_stages.hip launches the stages exactly as csrc/bds_acq.hip does and does no arithmetic of its own; inputs
and references are tests/pfa6_cases.py's, proven to be what they claim on the CPU by tests/test_pfa6_cases.py.

Every driver run is a child process under its own time limit.  A run that ends by signal, by time limit or with a HIP error marks the
module: every later test fails at once without starting another GPU process.  Nothing is retried.

Tolerances, all against the float64 reference, in the forms of tests/test_pfa32_stages_gpu.py (measured values:
profiles/pfa6_stage_errors.txt; each test prints what it measures):
  column pass   fp32 arithmetic.  Per lag sum_c w_c (sqrt(m_c + EPS S_c) - sqrt(m_c)) + 1e-6 a (pfa6_cases.ColsCell.value_tolerance),
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

import pfa6_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BUDGET = 1e-5
# 4 x the measured values of profiles/pfa6_stage_errors.txt (MI355X)
C_FWD = 4 * 1.841e-7   # measured 1.841e-7 (the batch of five signal spectra), 1.352e-7 (the code shape)
C_ROWS = 4 * 1.179e-7  # measured 1.179e-7 (p = 1, chunks of two), 9.189e-8, 8.763e-8, 1.104e-7
assert max(C_ROWS, C_FWD) <= BUDGET
# measured 8.919e-5 on the two value-mode cells (2.569e-7 on the noise cell alone): the finding of tests/test_pfa_stages_gpu.py at this
# size -- a floor-level output in the column (lag t3) of a peak hundreds of times the floor carries the fp32 error of the whole column
# (318 outputs), which the S of its mirror pair does not measure.  What a sieve decision can turn on is held to the budget itself: every
# lag at or above half the cell's maximum (measured 1.487e-7 of the maximum) and every value the sieve reports.
EPS_COLS = 4 * 8.919e-5
E2E_TOL = 1e-3         # measured worst 1.972e-4 of the maximum


def report(name, value):
    print(f"\npfa6_stage_errors: {name} = {value:.3e}")


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
    exe = os.environ.get("BDS_PFA6_STAGES_EXE")  # a prebuilt driver, e.g. one built against a modified header to see that the tests bite
    if not exe:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        if not os.path.exists(hipcc):
            pytest.skip("no hipcc on this box")
        exe = str(tmp_path_factory.mktemp("pfa6_stages") / "pfa6_stages")
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-fno-slp-vectorize",
               "-I" + os.path.join(ROOT, "bds-3-b1c-b2a-sdr-receiver_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
               os.path.join(ROOT, "tools", "probe", "pfa6_stages.hip"), "-o", exe]
        subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    return Driver(exe)


# ---- forward transforms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb, doubled, conj, stride", [(5, 1, 0, 2 * pc.NP), (2, 0, 1, pc.NP)], ids=["signal", "codes"])
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
    worst = 0.0
    for i in range(n):
        w = pc.bw_unpack_words(buf[g + i * pc.CELL_ELEMS:g + (i + 1) * pc.CELL_ELEMS])
        assert np.all(w[:, :, :, pc.K3:] == 0xFFFFFFFF)  # the pad lags of the last tile: never written
        body = w[:, :, :, :pc.K3]
        assert not np.any(body == 0xFFFFFFFF)  # every element of the cell written
        got = pc.unpack_h2(body)
        assert np.all(got[:, pc.K1] == 0)  # the pad row k1 = 53: exactly zero
        spec, s = pc.cell_of_bin(run.bins[i], run.p, run.q)
        ref = pc.rows_reference(spec, s, run.slots[i])
        worst = max(worst, pc.measure_c(got[:, :pc.K1], ref))
        tr, ti = pc.storage_tolerance(ref, C_ROWS)
        bad = (np.abs(got[:, :pc.K1].real - ref.real) > tr) | (np.abs(got[:, :pc.K1].imag - ref.imag) > ti)
        assert not np.any(bad), (i, run.bins[i], np.argwhere(bad)[:5])
    report(f"rows[{run.name}] c", worst)


# ---- column pass ----------------------------------------------------------------------------------------------------------------
def split_launches(res, launches):
    assert len(res) == 5 * len(launches)
    return [pc.parse_cols(res[5 * i:5 * i + 5]) for i in range(len(launches))]


def sieve_tolerance(cell, pos):
    """What a value the sieve reports may differ by: the per-lag tolerance, and never more than the budget of the cell's maximum."""
    return np.minimum(cell.value_tolerance(EPS_COLS, pos), BUDGET * cell.max)


def check_entries(r, cells, launch, positions_out=None, cell_of=None):
    """Every entry of the list: a cell of the launch, a lag of the cell at most once, the reference's value at that lag.  cell_of: the
    buffer cell behind listed cell i (masked launches with sources)."""
    _, inv = pc.lag_grid()
    e = r.entries
    local = e["cell"].astype(np.int64) - launch.cell0
    assert np.all((local >= 0) & (local < launch.ncells))
    assert np.all((e["lag"] >= 0) & (e["lag"] < pc.NP))
    for i in range(launch.ncells):
        cell = cells[i if cell_of is None else cell_of[i]]
        sel = e[local == i]
        pos = inv[sel["lag"]]
        assert len(np.unique(pos)) == len(pos), (cell.name, "a lag is listed twice")
        err = np.abs(sel["v"].astype(np.float64) - cell.a.reshape(-1)[pos])
        tol = sieve_tolerance(cell, pos)
        assert np.all(err <= tol), (cell.name, float(np.max(err / tol)))
        if positions_out is not None:
            positions_out.append(pos)


_required = {}


def required(cell, gmax, keep):
    key = (cell.name, gmax, keep)
    if key not in _required:
        _required[key] = pc.required_and_band(cell, gmax, keep)
    return _required[key]


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
    gm = pc.group_maxima(cells, launch.cell0, launch.lb_div)
    assert not np.any(r.cellmax_v[:launch.cell0])  # the slots of other launches' cells: untouched
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
        req, band = required(cell, gm[i], launch.keep)
        assert band == 0
        missing = np.setdiff1d(req, listed[i])
        assert not len(missing), (cell.name, len(missing), "required lags are not listed, e.g. grid position", int(missing[0]))
    # the running bound of a group ends as the largest of its cells' maxima
    for i in range(n):
        s = (launch.cell0 + i) // launch.lb_div
        group = [launch.cell0 + j for j in range(n) if (launch.cell0 + j) // launch.lb_div == s]
        assert r.lb[s] == max(r.cellmax_v[group])


def test_cols_value_mode(driver, tmp_path):
    """keep = 0 with the bounds zeroed: the list holds each of the N lags of each cell exactly once, ex.v the sieve value -- lag_of,
    t2_of, the t1 >= 53 and t3 >= 625 masks, the hi + lo coefficients, the row mapping of the three MFMA row groups, the 6-point stage and
    the S +- X epilogue, at every output."""
    cells = [pc.cell_noise(), pc.cell_edges()]
    launch = pc.Launch(2, 0, 1, 1, pc.host_grid(2, 1), 2 * pc.NP, True, 0.0)
    (r,) = split_launches(driver.run(pc.cols_case(cells, [launch]), tmp_path, timeout=90), [launch])
    assert pc.guard_intact(r.head_guard) and pc.guard_intact(r.tail_guard)
    assert r.count == 2 * pc.NP and len(r.entries) == r.count
    assert r.stats[0] == 2 * pc.WAVE_ITEMS_PER_CELL and r.stats[1] == pc.NBLOCKS * r.stats[0]  # every output block of every wave item listed
    _, inv = pc.lag_grid()
    eps = upper = 0.0
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
        assert np.all(err <= tol), (cell.name, int(np.argmax(err / tol)), float(np.max(err / tol)))
        # the lags a sieve decision can turn on -- the upper half of the cell's values -- to the budget of the maximum
        assert np.all(err[high] <= BUDGET * cell.max)
        lag = int(r.cellmax_lag[i])
        tol = np.minimum(tol, BUDGET * cell.max)
        assert abs(float(r.cellmax_v[i]) - cell.max) <= tol[int(np.argmax(cell.a))] and cell.a.reshape(-1)[inv[lag]] >= cell.max - tol[inv[lag]]


SINGLE = {"noise": pc.cell_noise, "near": pc.cell_near, "tie": pc.cell_tie}


@pytest.mark.parametrize("name", list(SINGLE))
def test_cols_sieve_single_cell(driver, tmp_path, name):
    """keep = 0.996 as shipped.  A grid of 7 walks the tiles nearly in order (the threshold of a cell is set before its later tiles
    are judged against it); the host's own grid has every tile of the cell in flight at once."""
    cell = SINGLE[name]()
    launches = [pc.Launch(1, 0, 1, q, g, 1 << 16, True, pc.KEEP) for q, g in ((1, 7), (1, pc.host_grid(1, 1)), (4, pc.host_grid(1, 4)))]
    results = split_launches(driver.run(pc.cols_case([cell], launches), tmp_path), launches)
    lag_grid = pc.lag_grid()[0]
    for launch, r in zip(launches, results):
        check_sieve(r, [cell], launch)
        listed = set(r.entries["lag"].tolist())
        if name == "near":
            for p, q, above in cell.notes["pairs"]:  # pairs that share a lane: both listed when both are above the threshold
                assert int(lag_grid[p]) in listed and (not above or int(lag_grid[q]) in listed)
        if name == "tie":  # all 318 tie in fp32 too: the smallest of their lags, and all of them listed
            lags = lag_grid[:, :, pc.TIE_T3].ravel()
            assert int(r.cellmax_lag[0]) == int(lags.min())
            assert listed.issuperset(lags.tolist())
            tied = r.entries[np.isin(r.entries["lag"], lags)]["v"]
            assert len(tied) == 318 and np.all(tied == r.cellmax_v[0])


def test_cols_sieve_multi_cell(driver, tmp_path):
    """ncells x qchunk x grid, cell0 = 3, two cells per running bound: the work list walked in its three digits."""
    cells = [f() for f in pc.MULTI_CELLS]
    launches = pc.multi_launches()
    assert len(launches) == 36
    results = split_launches(driver.run(pc.cols_case(cells, launches), tmp_path, timeout=90), launches)
    for launch, r in zip(launches, results):
        try:
            check_sieve(r, cells, launch)
        except AssertionError as e:
            raise AssertionError(f"{launch}: {e}") from e


def test_cols_list_overflow(driver, tmp_path):
    """A list shorter than the qualifying lags: the counter runs past the capacity, the slots hold valid entries, nothing behind them."""
    cell = pc.cell_near()
    cap = 100
    assert cap < cell.claims
    launch = pc.Launch(1, 0, 1, 1, pc.host_grid(1, 1), cap, True, pc.KEEP)
    (r,) = split_launches(driver.run(pc.cols_case([cell], [launch]), tmp_path), [launch])
    assert r.count >= cell.claims > cap and len(r.entries) == cap
    assert pc.guard_intact(r.head_guard) and pc.guard_intact(r.tail_guard)
    assert np.all(r.entries["v"] > 0)  # every slot taken (the list is prefilled with zeros)
    check_entries(r, [cell], launch)


def test_cols_masked(driver, tmp_path):
    """k_pfa6_cols<true> as the second-peak pass launches it: four listed cells with their own lag ranges, the rows read from buffer cells
    src = (1, 1, 0, 1) (the buffer holds the noise cell and the masked cell).  keep = 0: every lag INSIDE a range comes back exactly once
    with its value, no lag outside one -- inclusive at lo and hi (edges on peaks), a peak one lag outside never listed; an entry with an
    empty first range; an entry with both ranges empty reports nothing at all.  Then keep = 0.996 on the same lists: the sieve contract
    restricted to the ranges, and the same launch with identity sources (src = none) on a buffer of four cells."""
    cells = [pc.cell_noise(), pc.cell_masked()]
    rngs = pc.mask_ranges()
    src = [1, 1, 0, 1]
    n = len(rngs)
    grid = pc.host_grid(n, 1)
    launches = [pc.Launch(n, 0, 1, 1, grid, n * pc.NP, True, 0.0, True), pc.Launch(n, 0, 1, 1, grid, 1 << 16, True, pc.KEEP, True),
                pc.Launch(n, 2, 1, 4, 7, 1 << 16, True, pc.KEEP, True)]
    results = split_launches(driver.run(pc.cols_case(cells, launches, rngs, src, n), tmp_path, timeout=90), launches)
    _, inv = pc.lag_grid()
    lag_grid = pc.lag_grid()[0].ravel()
    peaks = sorted(cells[1].notes["lags"])
    for launch, r in zip(launches, results):
        assert pc.guard_intact(r.head_guard) and pc.guard_intact(r.tail_guard)
        assert r.stats[0] == pc.WAVE_ITEMS_PER_CELL * n and len(r.entries) == r.count
        listed = []
        check_entries(r, cells, launch, listed, cell_of=src)
        for i in range(n):
            cell, allowed = cells[src[i]], pc.in_ranges(rngs[i])
            got = np.zeros(pc.NP, dtype=bool)
            got[listed[i]] = True
            assert not np.any(got & ~allowed), (i, "a lag outside the ranges is listed")
            slot = launch.cell0 + i
            if not allowed.any():
                assert r.cellmax_v[slot] == 0 and r.lb[slot] == 0 and not got.any()
                continue
            a = np.where(allowed, cell.a.reshape(-1), -1.0)
            top = int(np.argmax(a))
            if launch.keep == 0.0:
                assert np.array_equal(got, allowed), (i, "every lag inside the ranges, once")
            else:
                req, band = pc.required_and_band(cell, a[top], launch.keep, allowed)
                assert band == 0 and got[req].all()
            v, lag = float(r.cellmax_v[slot]), int(r.cellmax_lag[slot])
            assert abs(v - a[top]) <= sieve_tolerance(cell, np.array([top]))[0] and allowed[inv[lag]]
            assert a[inv[lag]] >= a[top] - sieve_tolerance(cell, np.array([inv[lag]]))[0]
            assert r.lb[slot] == r.cellmax_v[slot]
    # the edges, spelled out on the value-mode launch: ranges (L0..L1, L2+1..L3-1) list L0 and L1, not L2 and L3
    first = set(lag_grid[listed_of(results[0], 0)].tolist())
    assert peaks[0] in first and peaks[1] in first and peaks[2] not in first and peaks[3] not in first
    second = set(lag_grid[listed_of(results[0], 1)].tolist())
    assert peaks[4] in second and peaks[5] in second and peaks[1] not in second and peaks[2] not in second
    assert set(lag_grid[listed_of(results[0], 2)].tolist()) == {peaks[3]}
    # identity sources: the listed cell i reads buffer cell i
    cells4 = [pc.cell_masked(), pc.cell_noise(), pc.cell_masked(), pc.cell_noise()]
    launch = pc.Launch(n, 0, 1, 1, grid, n * pc.NP, True, 0.0, True)
    (r,) = split_launches(driver.run(pc.cols_case(cells4, [launch], rngs, None, n), tmp_path, timeout=90), [launch])
    listed = []
    check_entries(r, cells4, launch, listed)
    for i in range(n):
        got = np.zeros(pc.NP, dtype=bool)
        got[listed[i]] = True
        assert np.array_equal(got, pc.in_ranges(rngs[i]))


def listed_of(r, i):
    """grid positions of the entries of listed cell i (cell0 = 0)"""
    return pc.lag_grid()[1][r.entries[r.entries["cell"] == i]["lag"]]


# ---- the pair ---------------------------------------------------------------------------------------------------------------------
def test_pair_end_to_end(driver, tmp_path):
    """Rows, then columns in value mode on the device's own buffer, against numpy.fft of the natural-order spectra at every lag: the
    index maps, the spectrum index (bin 821 = 5 x 164 + 1: spectrum 1), the rotation (4 x 164 = 656: past 625, and 656 mod 53, mod 6 and
    mod 625 all differ) and the fp16 storage together."""
    run = pc.RowsRun("pair", (821,), (1,), 1, 4, 5)
    assert pc.cell_of_bin(821, 4, 5) == (1, 656)
    launch = pc.Launch(1, 0, 1, 1, pc.host_grid(1, 1), pc.NP, True, 0.0)
    res = driver.run(pc.rows_case(run, [launch], write_bw=False), tmp_path, timeout=90)
    assert pc.guard_intact(res[0])
    (r,) = split_launches(res[1:], [launch])
    assert r.count == pc.NP and np.array_equal(np.sort(r.entries["lag"]), np.arange(pc.NP))
    got = np.empty(pc.NP)
    got[r.entries["lag"]] = r.entries["v"]
    ref = pc.e2e_reference(1, 656, 1)
    worst = float(np.max(np.abs(got - ref)) / ref.max())
    report("pair end to end, worst |error| / maximum", worst)
    assert worst <= E2E_TOL
    assert int(r.cellmax_lag[0]) == int(np.argmax(ref)) or ref[int(r.cellmax_lag[0])] >= ref.max() * (1 - E2E_TOL)
