"""The twiddle table of the N-point row passes (csrc/bds_tw3125.h, written by tools/gen_tw3125.py): every entry is the float64 cosine /
sine of 2 pi n / 3125 rounded once to fp32, bit for bit, and the header is what its generator writes.  The entries are read by parsing
the header: its literals are hexadecimal, so the text names the fp32 values exactly."""
import importlib.util
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "bds-3-b1c-b2a-sdr-receiver_amd", "csrc", "bds_tw3125.h")
K3 = 3125


def parse_header():
    with open(HEADER) as f:
        src = f.read()
    body = src[src.index("kTw3125[kTw3125Len][2] = {"):]
    rows = re.findall(r"^\s*\{(-?0x[0-9a-f.]+p[+-]\d+)f, (-?0x[0-9a-f.]+p[+-]\d+)f\},\s*// (\d+)$", body, flags=re.M)
    assert [int(r[2]) for r in rows] == list(range(K3))
    assert body.count("{") == K3 + 1  # nothing in the initialiser but the rows the pattern matched
    c = np.array([float.fromhex(r[0]) for r in rows])
    s = np.array([float.fromhex(r[1]) for r in rows])
    return c, s


def test_every_entry_is_the_float64_value_rounded_once():
    c, s = parse_header()
    # the literals are fp32 values: nothing is lost when the compiler reads them as float
    assert np.array_equal(c, np.float32(c).astype(np.float64)) and np.array_equal(s, np.float32(s).astype(np.float64))
    n = np.arange(K3)
    want_c = np.float32(np.cos(2 * np.pi * n / K3))
    want_s = np.float32(np.sin(2 * np.pi * n / K3))
    assert want_c.dtype == np.float32 and (2 * np.pi * n / K3).dtype == np.float64
    assert np.array_equal(np.float32(c).view(np.uint32), want_c.view(np.uint32))
    assert np.array_equal(np.float32(s).view(np.uint32), want_s.view(np.uint32))
    assert c[0] == 1.0 and s[0] == 0.0


def test_header_is_what_the_generator_writes():
    spec = importlib.util.spec_from_file_location("gen_tw3125", os.path.join(ROOT, "tools", "gen_tw3125.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(HEADER) as f:
        assert f.read() == gen.text()


def test_kernel_indices_stay_inside_the_table():
    """k_pfa_rows indexes the table without a reduction: j p (j <= 124, p <= 24) and 25 i u (i <= 24, u <= 4)."""
    assert 124 * 24 < K3 and 25 * 24 * 4 < K3
