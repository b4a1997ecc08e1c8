"""k_pfa_rows<2> (csrc/bds_acq_pfa.h) launched with a chunk table, against float64 at every output and against the uniform launch of
the same cells bit for bit.  tools/probe/pfa_rows_chunks.hip runs both launches, each into a guarded buffer of its own; inputs,
references and the tolerance are tests/pfa_cases.py's and the constant C of tests/test_pfa_stages_gpu.py (4 x 1.410e-7).

The shapes are the smallest at which the table indexing and the store path of the last row pair can go wrong: a non-uniform list with
chunks of one cell, the code slot changing from chunk to chunk, and rotations s = bin x shift in {0, 1, 11, 12, 52, 53, 200} (shift 1)
and {400, 12, 52} (shift 2), for which (k2 - s) mod 12 and (k1 - s) mod 53 wrap differently in the two halves of the workgroups of the
last row pair -- those hold row 52 of k2 and of k2 + 1, no longer rows 52 and 53 of one k2.

The driver runs as a child process under its own time limit.  A run that ends by signal, by time limit or with a HIP error marks the
module: every later test fails at once without starting another GPU process.  Nothing is retried."""
import os
import shutil
import subprocess
from collections import namedtuple

import numpy as np
import pytest

import pfa_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_ROWS = 4 * 1.410e-7  # tests/test_pfa_stages_gpu.py

ChunkRun = namedtuple("ChunkRun", "name bins slots chunks shift")
RUNS = (
    ChunkRun("mixed", (0, 1, 11, 12, 52, 53, 200), (0, 0, 0, 1, 1, 0, 1), (3, 2, 1, 1), 1),
    ChunkRun("shift2", (200, 6, 26), (1, 1, 0), (2, 1), 2),
)


def chunk_case(run):
    """The arrays of tools/probe/pfa_rows_chunks.hip: pfa_cases.rows_case's inputs, the header of stage 4 and the chunk table."""
    n = len(run.bins)
    assert sum(run.chunks) == n
    first = np.concatenate(([0], np.cumsum(run.chunks)[:-1]))
    for f, c in zip(first, run.chunks):
        assert len(set(run.slots[f:f + c])) == 1  # one PRN per chunk
    base = pc.rows_case(pc.RowsRun(run.name, run.bins, run.slots, 1, run.shift))
    header = np.array([pc.MAGIC, 4, n, 1, run.shift, pc.NSLOTS, pc.ROWS_GUARD], dtype=np.int64)
    table = np.stack([first, np.array(run.chunks)], axis=1).astype(np.int32)
    return [header] + base[1:5] + [table]


class Driver:
    def __init__(self, exe):
        self.exe = exe
        self.broken = None

    def run(self, arrays, tmp_path, timeout=90):
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
    exe = os.environ.get("BDS_PFA_ROWS_CHUNKS_EXE")  # a prebuilt driver
    if not exe:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        assert os.path.exists(hipcc), "the driver is built with hipcc"
        exe = str(tmp_path_factory.mktemp("pfa_rows_chunks") / "pfa_rows_chunks")
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-fno-slp-vectorize",
               "-I" + os.path.join(ROOT, "bds-3-b1c-b2a-sdr-receiver_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
               os.path.join(ROOT, "tools", "probe", "pfa_rows_chunks.hip"), "-o", exe]
        subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    return Driver(exe)


@pytest.mark.parametrize("run", RUNS, ids=lambda r: r.name)
def test_rows_with_chunk_table(driver, tmp_path, run):
    listed, uniform = (b.view(np.uint32) for b in driver.run(chunk_case(run), tmp_path))
    n, g = len(run.bins), pc.ROWS_GUARD
    assert listed.size == uniform.size == n * pc.CELL_ELEMS + 2 * g
    for buf in (listed, uniform):
        assert pc.guard_intact(buf[:g]) and pc.guard_intact(buf[-g:])
    worst = 0.0
    for i in range(n):
        w = pc.bw_unpack_words(listed[g + i * pc.CELL_ELEMS:g + (i + 1) * pc.CELL_ELEMS])
        assert np.all(w[:, :, :, pc.K3:] == 0xFFFFFFFF)  # the pad lags of the last tile: never written
        body = w[:, :, :, :pc.K3]
        assert not np.any(body == 0xFFFFFFFF)  # every element of the cell written
        assert not np.any(body[:, pc.K1])  # the pad row k1 = 53: zero words, not only zero values
        got = pc.unpack_h2(body)
        ref = pc.rows_reference(run.bins[i] * run.shift, run.slots[i])
        worst = max(worst, pc.measure_c(got[:, :pc.K1], ref))
        tr, ti = pc.storage_tolerance(ref, C_ROWS)
        bad = (np.abs(got[:, :pc.K1].real - ref.real) > tr) | (np.abs(got[:, :pc.K1].imag - ref.imag) > ti)
        assert not np.any(bad), (i, run.bins[i], np.argwhere(bad)[:5])
    print(f"\npfa_stage_errors: rows[chunks {run.name}] c = {worst:.3e}")
    # the output does not depend on the chunking
    assert np.array_equal(listed, uniform)
