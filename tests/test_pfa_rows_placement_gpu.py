"""k_pfa_rows<2> (csrc/bds_acq_pfa.h) under its banded placement (328 workgroups per chunk of cells, 10 of them idle) and its padded LDS
rows, against float64 at every output.  One run of tools/probe/pfa_rows_chunks.hip launches the row pass twice for the same three
cells, each into a guarded buffer of its own: with a chunk table (2 + 1 cells: chunk = blockIdx.x / 328 indexes the table) and in
uniform chunks of two cells (a short last chunk).  The cells are the bins 0, 200 (the last of the search band) and 65, whose rotation
wraps both the 53-point dimension (65 mod 53 = 12) and the 12-point one (65 mod 12 = 5); the PRN slot changes with the chunk.

Assertions as tests/test_pfa_stages_gpu.py::test_rows, per route: every element of every cell written, the pad row k1 = 53 exactly
zero, the pad lags of the last tile untouched, the guards intact, and every output within storage_tolerance at C_ROWS (inputs,
references and tolerance: tests/pfa_cases.py, tests/test_pfa_stages_gpu.py); then the two routes bit for bit.

The driver runs as a child process under its own time limit; nothing is retried after a failure."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pfa_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_ROWS = 4 * 1.410e-7  # tests/test_pfa_stages_gpu.py

BINS, SLOTS, CHUNKS, GC, SHIFT = (0, 200, 65), (0, 0, 1), (2, 1), 2, 1


def case():
    """The arrays of tools/probe/pfa_rows_chunks.hip: pfa_cases.rows_case's inputs, the header of stage 4 and the chunk table."""
    n = len(BINS)
    first = np.concatenate(([0], np.cumsum(CHUNKS)[:-1]))
    assert sum(CHUNKS) == n and all(len(set(SLOTS[f:f + c])) == 1 for f, c in zip(first, CHUNKS))  # one PRN per chunk
    assert all(len(set(SLOTS[c0:c0 + GC])) == 1 for c0 in range(0, n, GC))
    base = pc.rows_case(pc.RowsRun("placement", BINS, SLOTS, GC, SHIFT))
    header = np.array([pc.MAGIC, 4, n, GC, SHIFT, pc.NSLOTS, pc.ROWS_GUARD], dtype=np.int64)
    table = np.stack([first, np.array(CHUNKS)], axis=1).astype(np.int32)
    return [header] + base[1:5] + [table]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = os.environ.get("BDS_PFA_ROWS_CHUNKS_EXE")  # a prebuilt driver
    if not path:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        assert os.path.exists(hipcc), "the driver is built with hipcc"
        path = str(tmp_path_factory.mktemp("pfa_rows_placement") / "pfa_rows_chunks")
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-fno-slp-vectorize",
               "-I" + os.path.join(ROOT, "bds-3-b1c-b2a-sdr-receiver_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
               os.path.join(ROOT, "tools", "probe", "pfa_rows_chunks.hip"), "-o", path]
        subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    return path


@pytest.fixture(scope="module")
def buffers(exe, tmp_path_factory):
    """(listed, uniform): one child process, its own time limit."""
    tmp = tmp_path_factory.mktemp("pfa_rows_placement_run")
    cfile, out = str(tmp / "case.bin"), str(tmp / "out.bin")
    pc.write_arrays(cfile, case())
    try:
        r = subprocess.run([exe, cfile, out], capture_output=True, text=True, timeout=90)
    finally:
        os.remove(cfile)
    assert r.returncode == 0 and "ok" in r.stdout, f"driver exit status {r.returncode}: {r.stderr.strip()[-400:]}"
    res = pc.read_arrays(out)
    os.remove(out)
    assert len(res) == 2
    return tuple(b.view(np.uint32) for b in res)


@pytest.fixture(scope="module")
def references():
    return [pc.rows_reference(b * SHIFT, s) for b, s in zip(BINS, SLOTS)]


@pytest.mark.parametrize("route", [0, 1], ids=["chunk_list", "uniform"])
def test_rows_of_every_cell(buffers, references, route):
    buf = buffers[route]
    n, g = len(BINS), pc.ROWS_GUARD
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
        ref = references[i]
        worst = max(worst, pc.measure_c(got[:, :pc.K1], ref))
        tr, ti = pc.storage_tolerance(ref, C_ROWS)
        bad = (np.abs(got[:, :pc.K1].real - ref.real) > tr) | (np.abs(got[:, :pc.K1].imag - ref.imag) > ti)
        assert not np.any(bad), (i, BINS[i], np.argwhere(bad)[:5])
    print(f"\npfa_stage_errors: rows[placement {'chunk list' if route == 0 else 'uniform'}] c = {worst:.3e}")


def test_routes_agree_bit_for_bit(buffers):
    assert np.array_equal(buffers[0], buffers[1])
