"""Inputs and float64 references of every stage of the opt-in N-point search pair for B1C at 30.69 MS/s (csrc/bds_acq_pfa31.h), built on
the NumPy model tools/proto_pfa31.py: one synthetic block at init_settings_b1c(samplingFreq=30.69e6, IF=7.5e6), the signal spectrum of
bin 0 and the code spectra of one PRN in the kernels' layouts, the inter-pass values and the |y|^2 of a cell -- each stage's reference is
the next stage's input, and tests/test_pfa31_cases.py proves on the CPU that they compose to the direct N-point correlation and to the
oracle's results(bin, :)."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import proto_pfa31 as pp  # noqa: E402

NP, K1, K2, K3 = pp.N, pp.K1, pp.K2, pp.K3
FS, IF, BAND, STEP = 30.69e6, 7.5e6, 250.0, 50.0
SPC = 306900
PRN = 19
DOPPLER_BIN = 7          # the satellite sits on bin 7 of the 11: -250 + 7 x 50 = +100 Hz
W0, W1 = np.sqrt(11.0 / 40.0), np.sqrt(29.0 / 40.0)  # B1C/acquisition.m:216-219


def settings():
    import bds_amd

    return bds_amd.init_settings_b1c(samplingFreq=FS, IF=IF, acqSearchBand=BAND, acqSatelliteList=[PRN])


@functools.lru_cache(maxsize=None)
def block():
    """4 x spc int8 samples: PRN 19 at +100 Hz, 45 dB-Hz"""
    from bds_amd import synth

    s = settings()
    return synth.make_if(s, [synth.Sat(PRN, -BAND + STEP * DOPPLER_BIN, 0.613 * SPC, 0.7, 45.0)], 4 * SPC, seed=31)


def shift():
    """spectrum bins per Doppler bin: acqStep N / fs"""
    sh = STEP * NP / FS
    assert sh == 1.0
    return int(sh)


@functools.lru_cache(maxsize=None)
def signal_rows():
    """forward reference, signal shape: the spectrum of carr_0 x in rows [31][11][1800], natural k3 order (B1C/acquisition.m:198-205)"""
    x = block()[:NP].astype(np.float64)
    k = np.arange(NP, dtype=np.int64)
    f0 = int(IF - BAND)
    carr = np.exp(2j * np.pi * ((f0 * k) % int(FS)) / FS)  # exp(1i f0 phasePoints), the turn count reduced exactly
    return pp.forward(carr * x)


@functools.lru_cache(maxsize=None)
def code_rows():
    """forward reference, code shape: conj(fft([table(1:X) zeros])) / N of the data and the pilot component (:176-187), rows [2][31][11][1800]"""
    from oracle import codes

    s = settings()
    x_len = NP // 2
    out = []
    for tab in (codes.make_data_table(s, PRN), codes.make_pilot_table(s, PRN)):
        c = np.concatenate([np.asarray(tab[:x_len], dtype=np.float64), np.zeros(NP - x_len)])
        out.append(np.conj(pp.forward(c)) / NP)
    return np.stack(out)


def inter_pass(b, **err):
    """row-pass reference of the cell of bin b: [2][31][11][1800] complex"""
    X, C = signal_rows(), code_rows()
    return np.stack([pp.inter_pass(X, C[c], b * shift(), **err) for c in range(2)])


def cell_values(b, **err):
    """column-pass reference in value mode: w_d |y_d| + w_p |y_p| over all lags [N]"""
    rows_err = {k: v for k, v in err.items() if k in ("plus", "swap_maps")}
    cols_err = {k: v for k, v in err.items() if k in ("missing_conj", "last_tile_of")}
    B = inter_pass(b, **rows_err)
    m = [np.sqrt(np.maximum(pp.column_pass(B[c], **cols_err), 0.0)) for c in range(2)]
    return W0 * m[0] + W1 * m[1]


def oracle_row(b):
    from oracle import acquisition as oacq

    (_, row), = oacq.b1c_coarse_rows(block().astype(np.float64), settings(), PRN, bins=[b])
    return row


def direct_correlation(b, lags):
    """the N-point circular correlation of carr_b x with both codes at a few lags, as direct float64 sums in natural order"""
    from oracle import codes

    s = settings()
    x = block()[:NP].astype(np.float64)
    k = np.arange(NP, dtype=np.int64)
    f = int(IF - BAND + STEP * b)
    y = np.exp(2j * np.pi * ((f * k) % int(FS)) / FS) * x
    x_len = NP // 2
    out = np.zeros(len(lags))
    for w, tab in ((W0, codes.make_data_table(s, PRN)), (W1, codes.make_pilot_table(s, PRN))):
        c = np.asarray(tab[:x_len], dtype=np.float64)
        for i, t in enumerate(lags):
            out[i] += w * abs(np.dot(y[(t + np.arange(x_len)) % NP], c))
    return out


# ---- cases of tools/probe/pfa31_stages.hip (tests/test_pfa31_stages_gpu.py) -------------------------------------------------------------
# Random inputs in the kernels' storage formats; the float64 references are the model's (tools/proto_pfa31.py), whose stages the CPU
# tests above tie to the direct correlation and the oracle.
from collections import namedtuple  # noqa: E402

from pfa_cases import (BAND as SIEVE_BAND, EXTRA_DT, GUARD_EXTRA, GUARD_WORD, KEEP, MAGIC, guard_intact, measure_c, pack_h2,  # noqa: E402,F401
                       parse_cols, read_arrays, round_h2, storage_tolerance, unpack_h2, write_arrays)
from pfa_cases import W0 as WK0, W1 as WK1  # noqa: E402  (the weights as the kernel holds them, fp32)

TILE, TILES, CELL_ELEMS = pp.TILE, pp.TILES, pp.CELL_ELEMS
WAVE_ITEMS_PER_CELL = (TILES - 1) * 4 + 2  # waves with t0 = 16 tile + 4 wave < 1800
NBLOCKS = pp.NB
ROWS_GUARD = TILE * K1 * K2 * 2            # elements in front of and behind the destination: one tile
FWD_SCALE = 1.0 / 65536.0
NSLOTS = 2
Launch = namedtuple("Launch", "ncells cell0 lb_div qchunk grid extra_cap stats keep")
RowsRun = namedtuple("RowsRun", "name bins slots gc shift")
# rotation 0, 1 and the largest of the 201-bin grid; a run of cells that crosses a PRN boundary (chunks of two: the second chunk starts
# on the other PRN's code rows and is short); two spectrum bins per Doppler bin (rotation 200 from bin 100)
ROWS_RUNS = (RowsRun("rot-0-1", (0, 1), (0, 0), 2, 1), RowsRun("prn-boundary", (3, 200, 0), (0, 0, 1), 2, 1),
             RowsRun("largest", (200,), (1,), 1, 1), RowsRun("shift-2", (100,), (0,), 1, 2))


def lag_grid():
    """(lag[t1, t2, t3], its inverse: grid position (flat index into [31][11][1800]) of every lag)."""
    lag = pp.lag_of(np.arange(K1)[:, None, None], np.arange(K2)[None, :, None], np.arange(K3)[None, None, :])
    inv = np.empty(NP, dtype=np.int64)
    inv[lag.ravel()] = np.arange(NP, dtype=np.int64)
    return lag, inv


def bw_pack(z):
    """z[2][31][11][1800] (fp16-exact values) -> a cell of the inter-pass buffer; the 8 pad lags of the last tile hold 0xffffffff (two
    fp16 NaNs): no kernel may read them."""
    full = np.full((2, K1, K2, TILES * TILE), 0xFFFFFFFF, dtype=np.uint32)
    full[:, :, :, :K3] = pack_h2(z)
    return np.ascontiguousarray(full.reshape(2, K1, K2, TILES, TILE).transpose(3, 1, 2, 4, 0)).reshape(-1)


def bw_unpack_words(cell):
    """A cell of the inter-pass buffer -> its words as [2][31][11][1808] (pad lags included)."""
    w = np.asarray(cell, dtype=np.uint32).reshape(TILES, K1, K2, TILE, 2)
    return np.ascontiguousarray(w.transpose(4, 1, 2, 0, 3)).reshape(2, K1, K2, TILES * TILE)


def launch_table(launches):
    return np.array([[l.ncells, l.cell0, l.lb_div, l.qchunk, l.grid, l.extra_cap, int(l.stats), l.keep, WK0, WK1] for l in launches], dtype=np.float64).reshape(-1, 10)


def host_grid(ncells, qchunk):
    """The column grid csrc/bds_acq.hip launches for a cell list of this size."""
    items = (TILES + qchunk - 1) // qchunk * qchunk * ncells
    return min(items, max(512, min(8192, items // 24)))


@functools.lru_cache(maxsize=None)
def forward_input():
    rng = np.random.default_rng(311)
    x = (rng.integers(-90, 91, size=(2, NP)) + 1j * rng.integers(-90, 91, size=(2, NP))).astype(np.complex64)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def forward_reference():
    """[2][31][11][1800]: the N-point spectra of the two inputs in natural k3 order, scaled"""
    return np.stack([pp.forward(x.astype(np.complex128)) for x in forward_input()]) * FWD_SCALE


def forward_case(nb, doubled, conj, stride):
    head = np.array([MAGIC, 1, nb, doubled, conj, stride], dtype=np.int64)
    return [head, np.array([FWD_SCALE]), np.ascontiguousarray(forward_input()[:nb]).view(np.float32)]


@functools.lru_cache(maxsize=None)
def rows_spectra():
    """(X[31][11][1800], C[NSLOTS][2][31][11][1800]) as fp16-exact complex values of the magnitudes a run stores"""
    rng = np.random.default_rng(312)
    X = round_h2(0.2 * (rng.standard_normal((K1, K2, K3)) + 1j * rng.standard_normal((K1, K2, K3))))
    C = round_h2(0.5 * (rng.standard_normal((NSLOTS, 2, K1, K2, K3)) + 1j * rng.standard_normal((NSLOTS, 2, K1, K2, K3))))
    return X, C


def rows_case(run, launches=(), write_bw=True):
    X, C = rows_spectra()
    head = np.array([MAGIC, 2, len(run.bins), run.gc, run.shift, NSLOTS, ROWS_GUARD, int(write_bw)], dtype=np.int64)
    xs = pack_h2(np.concatenate([X, X], axis=-1))
    return [head, xs, pack_h2(C), np.array(run.bins, dtype=np.int32), np.array(run.slots, dtype=np.int64) * (2 * NP), launch_table(launches)]


def rows_reference(s, slot):
    """[2][31][11][1800]: the inter-pass values of the cell rotated by s with the code rows of `slot`"""
    X, C = rows_spectra()
    return np.stack([pp.inter_pass(X, C[slot, c], s) for c in range(2)])


def e2e_reference(s, slot):
    """a[lag] = w0 |y_d| + w1 |y_p| over the N lags in natural order, from the unrounded inter-pass values"""
    B = rows_reference(s, slot)
    return WK0 * np.sqrt(pp.column_pass(B[0])) + WK1 * np.sqrt(pp.column_pass(B[1]))


class ColsCell:
    """One cell of the inter-pass buffer with its float64 reference: m[c][t1][t2][t3] = |y_c|^2 and a = w0 |y_d| + w1 |y_p| in grid order
    [31][11][1800], both from the ROUNDED buffer."""

    def __init__(self, name, z):
        self.name = name
        self.words = bw_pack(z)
        y = np.fft.ifft2(z, axes=(1, 2)) * (K1 * K2)
        self.m = y.real ** 2 + y.imag ** 2
        self.a = WK0 * np.sqrt(self.m[0]) + WK1 * np.sqrt(self.m[1])
        self.max = float(self.a.max())

    def value_tolerance(self, eps, idx=None):
        """Per lag (grid order; idx = flat grid positions, default all): the kernel forms |y|^2 of the pair (t2, 11 - t2) as S +- X, so the
        error of |y_c|^2 scales with S_c = |y_c[t2]|^2 + |y_c[11 - t2]|^2: sum_c w_c (sqrt(m_c + eps S_c) - sqrt(m_c)) + 1e-6 a."""
        m = self.m.reshape(2, -1)
        if idx is None:
            idx = np.arange(NP)
        t1, rem = np.divmod(idx, K2 * K3)
        t2, t3 = np.divmod(rem, K3)
        mirror = (t1 * K2 + (K2 - t2) % K2) * K3 + t3
        mc = m[:, idx]
        grow = np.sqrt(mc + eps * (mc + m[:, mirror])) - np.sqrt(mc)
        return WK0 * grow[0] + WK1 * grow[1] + 1e-6 * self.a.reshape(-1)[idx]

    def measure_eps(self, got_grid):
        """The smallest eps of value_tolerance that passes every lag (bisection; got_grid in grid order)."""
        a = self.a.reshape(-1)
        err = np.abs(got_grid - a)
        idx = np.nonzero(err > 1e-6 * a)[0]
        if not len(idx):
            return 0.0
        lo, hi = 0.0, 1e-6
        while np.any(err[idx] > self.value_tolerance(hi, idx)):
            lo, hi = hi, hi * 4
            if hi > 1.0:
                return float("inf")
        for _ in range(30):
            mid = 0.5 * (lo + hi)
            if np.any(err[idx] > self.value_tolerance(mid, idx)):
                lo = mid
            else:
                hi = mid
        return hi


def _cell(name, seed, peaks=()):
    """Lag-domain noise of unit floor with peaks (t1, t2, t3, a) planted, as the fp16-rounded buffer values"""
    rng = np.random.default_rng(seed)
    y = (rng.standard_normal((2, K1, K2, K3)) + 1j * rng.standard_normal((2, K1, K2, K3))) * np.sqrt(0.5)
    wsum2 = WK0 * WK0 + WK1 * WK1
    for t1, t2, t3, a in peaks:
        y[:, t1, t2, t3] = np.array([WK0, WK1]) * a / wsum2 * np.exp(2j * np.pi * rng.random(2))
    return ColsCell(name, round_h2(np.fft.fft2(y, axes=(1, 2)) / (K1 * K2)))


@functools.lru_cache(maxsize=None)
def cell_noise():
    return _cell("noise", 313)


@functools.lru_cache(maxsize=None)
def cell_peak():
    """one peak 300 times the floor, in the short last tile, at the last t1 and t2"""
    return _cell("peak", 314, [(30, 10, 1797, 300.0)])


@functools.lru_cache(maxsize=None)
def cell_edges():
    """peaks near one another in value (all above KEEP of the largest) on the edges of the three dimensions, of a wave's lags and of a tile"""
    return _cell("edges", 315, [(0, 0, 0, 300.0), (30, 10, 1799, 299.9), (15, 5, 15, 299.8), (1, 6, 16, 299.7), (29, 4, 1791, 299.6), (7, 1, 1792, 299.5),
                                (20, 9, 3, 299.4), (11, 2, 4, 299.3), (12, 0, 900, 200.0)])


def required(cell, gmax, keep):
    """grid positions a sieve launch must list: every lag at or above keep (1 + band) gmax; and how many lie in the ambiguity band below"""
    a = cell.a.reshape(-1)
    req = np.nonzero(a >= keep * (1 + SIEVE_BAND) * gmax)[0]
    band = int(np.count_nonzero((a >= keep * (1 - SIEVE_BAND) * gmax) & (a < keep * (1 + SIEVE_BAND) * gmax)))
    return req, band


def cols_case(cells, launches):
    head = np.array([MAGIC, 3, len(cells)], dtype=np.int64)
    return [head, np.concatenate([c.words for c in cells]), launch_table(launches)]
