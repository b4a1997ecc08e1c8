"""Every output of every kernel of the resampling conditioner (csrc/bds_resample.h) against its reference: k_ff_extend, k_ff_decimate and
k_widen16 bit for bit, k_ff_fir within the derived tolerance tol1 of a long-double evaluation, at every output, plus the identities
that hold as bits (tests/resample_cases.py has the references, the tolerance and the assertion functions; tests/test_resample_cases.py
shows on the CPU that those functions reject a kernel with one change).  tools/probe/resample_stages.hip launches the kernels with the
grid, block and LDS size of condition_block (csrc/bds_acq.hip) and does no arithmetic of its own.

Every driver run is a child process under its own time limit.  A run that ends by signal, by time limit or with a HIP error marks the
module: every later test fails at once without starting another GPU process.  Nothing is retried.  Each test prints the largest
error / tolerance it saw (0 where the check is bit for bit); the values measured on an MI355X are in profiles/resample_stage_errors.txt.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import resample_cases as rc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def report(name, value):
    print(f"\nresample_stage_errors: {name} = {value:.3e}")


class Driver:
    def __init__(self, exe):
        self.exe = exe
        self.broken = None

    def run(self, jobs, tmp_path, timeout=60, refused=False):
        """One child process: case file in, one result array per job out."""
        if self.broken:
            pytest.fail("no further GPU process after: " + self.broken)
        case, out = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
        rc.write_arrays(case, rc.case_file(jobs) if not refused else jobs)
        try:
            r = subprocess.run([self.exe, case, out], capture_output=True, text=True, timeout=timeout)
        except subprocess.TimeoutExpired:
            self.broken = f"the driver ran into its time limit of {timeout} s"
            pytest.fail(self.broken)
        finally:
            os.remove(case)
        if refused:  # the caller expects the refusal (status 3, before any launch)
            return r
        if r.returncode == 3:
            pytest.fail("malformed case: " + r.stderr)
        if r.returncode != 0 or "ok" not in r.stdout:
            self.broken = f"driver exit status {r.returncode}: {r.stderr.strip()[-400:]}"
            pytest.fail(self.broken)
        res = rc.read_arrays(out)
        os.remove(out)
        assert len(res) == len(jobs)
        return res


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = os.environ.get("BDS_RESAMPLE_STAGES_EXE")  # a prebuilt driver, e.g. one built against a modified header to see that the tests bite
    if not exe:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        if not os.path.exists(hipcc):
            pytest.skip("no hipcc on this box")
        exe = str(tmp_path_factory.mktemp("resample_stages") / "resample_stages")
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-fno-slp-vectorize",
               "-I" + os.path.join(ROOT, "bds-3-b1c-b2a-sdr-receiver_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
               os.path.join(ROOT, "tools", "probe", "resample_stages.hip"), "-o", exe]
        subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    return Driver(exe)


# ---- k_ff_extend ------------------------------------------------------------------------------------------------------------------
def test_extend_bit_exact(driver, tmp_path):
    """All four instantiations on nfact = 2100 with n = 2101 (the smallest legal block: the head reflection reads x[n - 1], the tail
    reflection x[0]), 2102, 4200, 5000, and nfact = 6 with n = 7; full-range values with the type's extremes at both ends; n = 530 000 for
    <1, int8_t> and <2, int16_t> (a second trip of the grid-stride loop)."""
    cases = rc.extend_cases()
    assert len(cases) == 22 and {(c.nch, c.width) for c in cases} == {(1, 8), (2, 8), (1, 16), (2, 16)}
    res = driver.run([rc.job_extend(c) for c in cases], tmp_path)
    for c, raw in zip(cases, res):
        rc.assert_extend(c, rc.split_output(raw, (c.x.shape[0] + 2 * c.nfact, c.nch)))
    report("k_ff_extend, 22 cases (bit for bit)", 0.0)


# ---- k_widen16 --------------------------------------------------------------------------------------------------------------------
def test_widen16_bit_exact(driver, tmp_path):
    xs = rc.widen_cases()
    assert [len(x) for x in xs] == [1, 255, 257, 600000] and all(x.min() == -32768 for x in xs) and all(x.max() == 32767 for x in xs[1:])
    res = driver.run([rc.job_widen(x) for x in xs], tmp_path)
    for x, raw in zip(xs, res):
        rc.assert_widen(x, rc.split_output(raw, (len(x),)))
    report("k_widen16, 4 cases (bit for bit)", 0.0)


# ---- k_ff_decimate ----------------------------------------------------------------------------------------------------------------
def test_decimate_bit_exact(driver, tmp_path):
    """z[i] = i (channel 1: i + 0.5), so the output names the index read: ceil((k / fs') fs) in that operation order, k = 0 -> 1, on the
    rate pairs and lengths that contain the k at which k (fs / fs'), k fs / fs' and k (1 / fs') fs give another index; nfact 0 and 2100;
    NCH 1 and 2; sig_len = 530 000 for the second trip."""
    cases = rc.decimate_cases()
    assert len(cases) == 17 and cases[-1].sig_len > 524288
    res = driver.run([rc.job_decimate(c) for c in cases], tmp_path)
    for c, raw in zip(cases, res):
        rc.assert_decimate(c, rc.split_output(raw, (c.sig_len, c.nch)))
    report("k_ff_decimate, 17 cases (bit for bit)", 0.0)


# ---- k_ff_fir ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_taps", rc.FIR_TAPS)
def test_fir_every_output(driver, tmp_path, n_taps):
    """fir1's symmetric taps and asymmetric random taps; len 1, n_taps - 1, n_taps, n_taps + 1, 3 n_taps, 6301; normal values of size 1e2 (two
    streams), a constant, a unit impulse at 0 (the clamp: the running sum of the taps), mid-block and len - 1 (the taps, bit for bit);
    forward and reverse, NCH 1 and 2.  Every output within tol1 = 1.01 n_taps 2^-53 sum |b| |u| of the long-double reference; reverse =
    flip(forward(flip)) and each channel of an NCH = 2 run = the NCH = 1 run, as bits."""
    groups = rc.fir_groups(n_taps)
    jobs = [(g, key, rev, u) for g in groups for key, rev, u in rc.fir_jobs(g)]
    res = driver.run([rc.job_fir(u, g.b, rev) for g, _, rev, u in jobs], tmp_path)
    by_group = {}
    for (g, key, _, u), raw in zip(jobs, res):
        by_group.setdefault(g.name, {})[key] = rc.split_output(raw, u.shape)
    worst = 0.0
    for g in groups:
        worst = max(worst, rc.assert_fir_group(g, by_group[g.name]))
    report(f"k_ff_fir, {n_taps} taps, {len(jobs)} runs: largest error / tol1", worst)


def test_fir_second_grid_stride_trip(driver, tmp_path):
    """len = 534 200 (530 000 + 2 x 2100), 701 asymmetric taps, NCH 1: forward, reverse, and forward of the flipped signal."""
    b, u = rc.fir_big()[:2]
    assert len(u) == 534200 > 2048 * 256 and len(b) == 701
    res = driver.run([rc.job_fir(u[:, None], b, 0), rc.job_fir(u[:, None], b, 1), rc.job_fir(u[::-1][:, None], b, 0)], tmp_path)
    f, r, ff = (rc.split_output(raw, (len(u),)) for raw in res)
    report("k_ff_fir, 701 taps, len 534 200: largest error / tol1", rc.assert_fir_big(f, r, ff))


# ---- the driver refuses what it cannot run safely -----------------------------------------------------------------------------
def test_driver_refuses_malformed_cases_before_any_launch(driver, tmp_path):
    c = rc.extend_cases()[0]
    d = rc.decimate_cases()[0]
    g = rc.fir_group("asym", 2, 3)
    good = rc.case_file([rc.job_extend(c)])
    bad = {
        "magic": [np.array([rc.MAGIC + 1, 1], dtype=np.int64)] + good[1:],
        "job count": [np.array([rc.MAGIC, 2], dtype=np.int64)] + good[1:],
        "n <= nfact": rc.case_file([[np.array([1, 1, 8, 2100, 2100], dtype=np.int64), c.x[:2100]]]),
        "x too short": rc.case_file([[np.array([1, 1, 8, 2101, 2100], dtype=np.int64), c.x[:2100]]]),
        "unknown stage": rc.case_file([[np.array([9, 1], dtype=np.int64), c.x]]),
        "no taps": rc.case_file([[np.array([2, 1, 3, 0, 0], dtype=np.int64), g.signals[0][:, None], np.zeros(0)]]),
        "taps beyond the LDS bound": rc.case_file([[np.array([2, 1, 3, 5000, 0], dtype=np.int64), g.signals[0][:, None], np.zeros(5000)]]),
        "z too short": rc.case_file([[np.array([3, 1, 0, d.sig_len, 100], dtype=np.int64), np.array([d.new_fs, d.old_fs]), np.zeros(100)]]),
    }
    for name, arrays in bad.items():
        r = driver.run(arrays, tmp_path, refused=True)
        assert r.returncode == 3 and "bad case" in r.stderr and "ok" not in r.stdout, (name, r.returncode, r.stderr)
        assert not os.path.exists(str(tmp_path / "out.bin")), name
