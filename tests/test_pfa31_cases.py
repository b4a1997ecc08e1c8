"""The float64 references of tests/pfa31_cases.py, stage by stage, are what they claim -- checked on the CPU: the forward references are the
N-point spectra in the kernels' layouts, the row-pass and column-pass references compose to the direct N-point correlation (direct sums
in natural order at a few lags) and to the oracle's results(bin, :) over all N lags, and the same models with ONE deliberate change each
-- a swapped index map, a missing conjugate, a rotation by +s instead of -s, the wrong tile for the last lags -- are rejected by the very
assertions that accept the model.  The public header declares the switch and a new context has it off."""
import os
import re

import numpy as np
import pytest

import pfa31_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = pc.DOPPLER_BIN
# fp64 throughout: the references agree with the oracle to rounding (1e-9 of the row's maximum leaves three orders of margin over the
# 1e-12 the transforms of N = 613 800 points reach)
TOL = 1e-9


@pytest.fixture(scope="module")
def oracle_row():
    return pc.oracle_row(BIN)


def _agrees(values, row):
    return np.max(np.abs(values - row)) <= TOL * row.max()


def test_forward_references_are_the_n_point_spectra():
    x = pc.block()[:pc.NP].astype(np.float64)
    k = np.arange(pc.NP, dtype=np.int64)
    X = np.fft.fft(np.exp(2j * np.pi * ((int(pc.IF - pc.BAND) * k) % int(pc.FS)) / pc.FS) * x)
    rows = pc.signal_rows()
    assert rows.shape == (pc.K1, pc.K2, pc.K3)
    assert np.max(np.abs(rows[k % pc.K1, k % pc.K2, k % pc.K3] - X)) <= 1e-10 * np.max(np.abs(X))
    C = pc.code_rows()
    assert C.shape == (2, pc.K1, pc.K2, pc.K3) and np.all(np.isfinite(C))


def test_stages_compose_to_the_oracle_row(oracle_row):
    v = pc.cell_values(BIN)
    assert v.shape == oracle_row.shape == (pc.NP,)
    assert _agrees(v, oracle_row)
    assert int(np.argmax(v)) == int(np.argmax(oracle_row))
    assert abs(int(np.argmax(v)) % pc.SPC - round(0.613 * pc.SPC)) <= 3  # the satellite of the block


def test_stages_compose_to_the_direct_correlation():
    v = pc.cell_values(BIN)
    peak = int(np.argmax(v))
    lags = [0, 1, pc.NP - 1, peak, pc.pp.lag_of(30, 10, 1799), pc.pp.lag_of(15, 5, 16), pc.pp.lag_of(0, 0, 1792)]
    d = pc.direct_correlation(BIN, lags)
    assert np.max(np.abs(v[lags] - d)) <= TOL * v.max()


@pytest.mark.parametrize("err", [dict(swap_maps=True), dict(missing_conj=True), dict(plus=True), dict(last_tile_of=0)],
                         ids=["swapped-index-map", "missing-conjugate", "rotation-by-plus-s", "wrong-tile-for-the-last-lags"])
def test_one_deliberate_change_is_rejected(oracle_row, err):
    assert not _agrees(pc.cell_values(BIN, **err), oracle_row)


def test_the_wrong_tile_only_moves_the_last_lags(oracle_row):
    v = pc.cell_values(BIN, last_tile_of=0)
    t3 = np.empty(pc.NP, dtype=np.int64)
    t1, t2, t3g = np.meshgrid(np.arange(pc.K1), np.arange(pc.K2), np.arange(pc.K3), indexing="ij")
    t3[pc.pp.lag_of(t1, t2, t3g)] = t3g
    ok = t3 < (pc.pp.TILES - 1) * pc.pp.TILE
    assert np.max(np.abs(v[ok] - oracle_row[ok])) <= TOL * oracle_row.max() and not _agrees(v[~ok], oracle_row[~ok])
    assert (~ok).sum() == 8 * pc.K1 * pc.K2


def test_header_declares_the_switch_and_it_is_off_after_create():
    h = open(os.path.join(ROOT, "include", "bds_mi355x.h")).read()
    assert re.search(r"BDS_API\s+int\s+bds_acq_set_b1c_npoint\s*\(\s*bds_ctx\s*\*\s*ctx\s*,\s*int\s+on\s*\)\s*;", h)
    assert "613 800" in h and "default 0 (off)" in h
    from bds_amd import native

    assert "bds_acq_set_b1c_npoint" in native.EXPORTS and hasattr(native.Context, "acq_set_b1c_npoint")
    import inspect

    import bds_amd

    assert inspect.signature(bds_amd.acquisition).parameters["b1c_npoint"].default is None
    src = open(os.path.join(ROOT, "bds-3-b1c-b2a-sdr-receiver_amd", "csrc", "bds_acq.hip")).read()
    assert re.search(r"bool\s+b1c_npoint\s*=\s*false\s*;", src)
    assert re.search(r"kind == 4 && !a\.b1c_npoint\) kind = 0", src)
    assert hasattr(native.lib(), "bds_acq_set_b1c_npoint")
