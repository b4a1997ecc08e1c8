"""bds_synth / bds_synth_file / bds_synth_noise on the device against the NumPy restatement (tests/synth_cases.py) and against
synth.make_if itself.

Records: B1C at 30.69 MS/s -- 30 samples per chip exactly, so with the nominal code rate the samples of the satellite at
delay 100.0 fall ON the chip boundaries, the adversarial case for floor(); the other satellite (-4321.5 Hz) starts its first code
period at sample 20000.25, so the samples before it are in period -1 -- and B2a at 99.375 MS/s with three entries, two of them one
PRN at different delays (multipath).  The references are computed once per module."""
import numpy as np
import pytest

import bds_amd
from bds_amd import synth

import synth_cases as sc
from packed_cases import pack_iq, quantise, uses_every_nibble

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
FIRST = 12345
SEED = 3550


def _b1c():
    s = bds_amd.init_settings_b1c(samplingFreq=30.69e6, IF=7.5e6)
    return s, [synth.Sat(3, 1250.0, 100.0, 0.7, 47.0), synth.Sat(27, -4321.5, 20000.25, 2.9, 44.0)], 2 * 306900 + 77


def _b2a():
    s = bds_amd.init_settings_b2a()
    sats = [synth.Sat(19, 310.0, 36768.75, 1.1, 47.0), synth.Sat(20, -200.0, 70556.25, 0.3, 45.0), synth.Sat(19, 310.0, 36775.5, 2.1, 41.0)]
    return s, sats, 3 * 99375 + 7


CASES = {"b1c": _b1c, "b2a": _b2a}


@pytest.fixture(scope="module")
def refs():
    """Restated records, made once: per case and code_doppler the clean complex record from FIRST on, and the noise."""
    out = {}
    for name, mk in CASES.items():
        s, sats, n = mk()
        for cd in ((False, True) if name == "b1c" else (True,)):
            out[name, cd] = sc.clean_record(s, sats, FIRST, n, seed=SEED, iq=True, code_doppler=cd)
        out[name, "noise"] = sc.noise_normals(SEED, np.arange(FIRST, FIRST + n, dtype=np.int64))
    return out


def _bound(s, sats):
    """8 eps sum(amp) 1.3: indices and th are bit-identical by construction, only sin / cos differ (about an ulp each, and
    |s_I| + |s_Q| <= 1.3 of the amplitude); a flipped chip or symbol would show as 2 amp."""
    return 8 * EPS * sc.amp_sum(s, sats) * 1.3


@pytest.mark.parametrize("name,cd", [("b1c", False), ("b1c", True), ("b2a", True)])
def test_clean_sum_at_an_offset_equals_restatement(ctx, refs, name, cd):
    s, sats, n = CASES[name]()
    got = synth.make_if_device(s, sats, n, seed=SEED, first_sample=FIRST, clean=True, code_doppler=cd)
    assert got.dtype == np.float64 and got.shape == (n,)
    if name == "b1c":  # the case is what it claims: period -1 occurs, and (nominal code rate) samples sit on chip boundaries
        assert np.floor((FIRST - sats[1].delay) * (1.023e6 / 30.69e6) / 10230) == -1
        assert s.samplingFreq / s.codeFreqBasis == 30.0 and (FIRST + 25 - sats[0].delay) % 30 == 0
    err = np.abs(got - refs[name, cd].real).max()
    print("%s code_doppler=%s: max |device - restatement| = %.3e (bound %.3e)" % (name, cd, err, _bound(s, sats)))
    assert err <= _bound(s, sats)


@pytest.mark.parametrize("kw", [{"code_doppler": False}, {}, {"pilot61_secondary": True}])
def test_clean_sum_from_the_start_equals_make_if(ctx, kw):
    """Format 0 against synth.make_if(clean=True) itself, with make_if's own symbol draws supplied."""
    s, sats, n = _b1c()
    ref = synth.make_if(s, sats, n, seed=5, clean=True, **kw)
    got = synth.make_if_device(s, sats, n, clean=True, symbols=sc.make_if_symbols(s, sats, n, 5), **kw)
    err = np.abs(got - ref).max()
    print("B1C %s: max |device - make_if| = %.3e (bound %.3e)" % (kw, err, _bound(s, sats)))
    assert err <= _bound(s, sats)


@pytest.mark.parametrize("name", ["b1c", "b2a"])
@pytest.mark.parametrize("iq_sign", [0, 1, -1])
def test_int8_records_equal_restatement(ctx, refs, name, iq_sign):
    """Formats 1 and 2: the int8 values are equal wherever the float64 value is farther than 1e-9 from a rounding boundary (the
    device / NumPy difference is ~ 20 x 8.6 x a few ulp = 1e-13); the restatement alone excludes at most 2 samples (expected
    n 2e-9 = 0.003), and an excluded value is off by at most 1."""
    s, sats, n = CASES[name]()
    cd = name != "b1c"
    z, (g_i, g_q) = refs[name, cd], refs[name, "noise"]
    if iq_sign:
        v = np.empty(2 * n)
        v[0::2], v[1::2] = z.real + 20.0 * g_i, (z.imag if iq_sign > 0 else -z.imag) + 20.0 * g_q
    else:
        v = z.real + 20.0 * g_i
    got = synth.make_if_device(s, sats, n, seed=SEED, first_sample=FIRST, iq_sign=iq_sign, code_doppler=cd)
    assert got.dtype == np.int8 and got.shape == v.shape
    ex = sc.near_boundary(v)
    assert ex.sum() <= 2
    want = sc.quantise8(v)
    np.testing.assert_array_equal(got[~ex], want[~ex])
    assert np.abs(got[ex].astype(np.int16) - want[ex]).max(initial=0) <= 1
    assert np.abs(got.astype(np.float64)).max() <= 127 and got.std() > 15  # noise of sigma 20, clipped symmetrically


def test_noise_stream_across_the_32_bit_carry(ctx):
    """2^16 draws from sample 2^33 - 5 on: the counter's low word wraps inside the run.  |g| <= 8.6 and log / sqrt / cos differ by
    a few ulp between the device and NumPy: absolute bound 1e-13."""
    first, n = 2 ** 33 - 5, 1 << 16
    g_i, g_q = ctx.synth_noise(SEED, first, n)
    r_i, r_q = sc.noise_normals(SEED, np.arange(first, first + n, dtype=np.int64))
    err = max(np.abs(g_i - r_i).max(), np.abs(g_q - r_q).max())
    print("noise: max |device - restatement| = %.3e" % err)
    assert err <= 1e-13
    assert np.abs(r_i).max() < 8.6 and abs(r_i.mean()) < 5 / np.sqrt(n)


@pytest.mark.parametrize("name", ["b1c", "b2a"])
@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_random_access_pieces_equal_one_call(ctx, name, fmt):
    """Sample n depends on n alone: [0, 4 097) + [4 097, 70 001) + [70 001, n) is the one-call record, bit for bit (format 3: even cuts)."""
    s, sats, n = CASES[name]()
    kw = {0: {"clean": True}, 1: {}, 2: {"iq_sign": 1}, 3: {"iq_sign": -1, "packed": True}}[fmt]
    cuts = [0, 4097, 70001, n] if fmt != 3 else [0, 4098, 70002, n - n % 2]
    whole = synth.make_if_device(s, sats, cuts[-1], seed=SEED, **kw)
    parts = [synth.make_if_device(s, sats, b - a, seed=SEED, first_sample=a, **kw) for a, b in zip(cuts[:-1], cuts[1:])]
    np.testing.assert_array_equal(np.concatenate(parts), whole)
    other = synth.make_if_device(s, sats, cuts[1], seed=SEED + 1, **kw)
    assert fmt == 0 or not np.array_equal(other, whole[:other.size])  # the seed matters (the clean sum has no noise; its symbols differ later)


@pytest.mark.parametrize("name", ["b1c", "b2a"])
def test_packed_record_is_the_quantised_iq_record(ctx, name):
    """Format 3 = pack_iq(quantise(format 2)) of tests/packed_cases.py, and every nibble value occurs in both halves of a byte."""
    s, sats, n = CASES[name]()
    n -= n % 2
    pairs = synth.make_if_device(s, sats, n, seed=SEED, first_sample=FIRST + 1, iq_sign=-1)
    packed = synth.make_if_device(s, sats, n, seed=SEED, first_sample=FIRST + 1, iq_sign=-1, packed=True)
    assert packed.dtype == np.uint8 and packed.size == n // 2
    np.testing.assert_array_equal(packed, pack_iq(quantise(pairs)))
    assert uses_every_nibble(packed)
    low = synth.make_if_device(s, sats, 4096, seed=SEED, iq_sign=-1, packed=True, threshold=5.0)
    np.testing.assert_array_equal(low, pack_iq(quantise(synth.make_if_device(s, sats, 4096, seed=SEED, iq_sign=-1), threshold=5.0)))


@pytest.mark.parametrize("fmt", [1, 2, 3])
def test_write_if_equals_make_if_device(ctx, tmp_path, fmt):
    """The file made in pieces of 65 536 + 32 samples (and of a size that is no multiple of anything) is the one-call record's bytes."""
    s, sats, n = _b2a()
    n -= n % 2
    kw = {1: {}, 2: {"iq_sign": -1}, 3: {"iq_sign": -1, "packed": True}}[fmt]
    want = synth.make_if_device(s, sats, n, seed=SEED, first_sample=FIRST + 1, **kw).tobytes()
    for piece in (65536 + 32, 100001, 0):
        path = tmp_path / ("r%d.bin" % piece)
        synth.write_if(str(path), s, sats, n, seed=SEED, first_sample=FIRST + 1, piece_samples=piece, **kw)
        assert path.read_bytes() == want, piece


def test_no_satellites_is_noise_alone(ctx):
    s, _, _ = _b2a()
    x = synth.make_if_device(s, [], 1 << 16, seed=9)
    g_i, _ = sc.noise_normals(9, np.arange(1 << 16, dtype=np.int64))
    v = 20.0 * g_i
    ex = sc.near_boundary(v)
    np.testing.assert_array_equal(x[~ex], sc.quantise8(v)[~ex])
    assert np.all(synth.make_if_device(s, [], 1000, clean=True) == 0)


def test_device_record_acquires_like_the_oracle(ctx):
    """End to end: a 993 750-sample B2a block in the cfg1_b2a geometry from the device generator, PRN 19 present and PRN 5 absent,
    through bds_amd.acquisition against the float64 oracle on the same block."""
    from helpers import spc_of
    from oracle import acquisition as oacq

    s = bds_amd.init_settings_b2a(acqSatelliteList=[5, 19], acqSearchBand=400, acqStep=400, fineNoncoh=7)
    spc = spc_of(s)
    sats = [synth.Sat(19, 310.0, 0.37 * spc, 1.1, 47.0), synth.Sat(20, -200.0, 0.71 * spc, 0.3, 45.0)]
    x = synth.make_if_device(s, sats, 10 * spc, seed=SEED)
    assert x.size == 993750
    got = bds_amd.acquisition(x, s)
    ref = oacq.acquisition_b2a(x.astype(np.float64), s)
    print("PRN 19: carrFreq", got.carrFreq[18], "codePhase", got.codePhase[18], "peakMetric", got.peakMetric[18], "| PRN 5 peakMetric", got.peakMetric[4])
    np.testing.assert_array_equal(got.codePhase, ref.codePhase)
    np.testing.assert_array_equal(got.carrFreq, ref.carrFreq)
    np.testing.assert_allclose(got.peakMetric, ref.peakMetric, rtol=1e-6, atol=0)
    assert got.carrFreq[18] != 0 and got.carrFreq[4] == 0  # PRN 19 detected, PRN 5 not
    assert abs(got.carrFreq[18] - (s.IF + 310.0)) <= 200 and abs(got.codePhase[18] - 0.37 * spc) <= 4
