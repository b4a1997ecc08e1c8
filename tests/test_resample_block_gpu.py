"""The conditioner as the library runs it: the float64 block the search reads after bds_acq_load* with the resampling branch on
(condition_block in csrc/bds_acq.hip: k_ff_extend, k_ff_fir forward and reverse, k_ff_decimate), fetched through the test aid
bds_acq_block, at EVERY sample against the long-double restatement of filtfilt + index decimation of tests/resample_cases.py, within
the derived two-pass tolerance tol2 -- on the smallest blocks bds_acq_load accepts, so that the tail reflection, the tail of both passes
and the last decimated samples are part of what is checked.  Every reference is computed once per module (I and Q filter
independently: an I/Q reference is two real ones) and left unchanged.  Each test prints the largest error / tol2 it saw
(profiles/resample_stage_errors.txt has the values measured on an MI355X).

(B1C at 40 -> 29 MS/s: the search transforms N' = 2 x 290 000 samples with acqCohT = 10, so the shortest accepted block has 800 001
samples, and its 580 000 decimation indices contain the k on which the neighbouring evaluation orders of the index part.)
"""
import functools

import numpy as np
import pytest
import torch

import bds_amd
from bds_amd import native

import resample_cases as rc
from helpers import resample_b1c, spc_of
from packed_cases import pack_iq, quantise, uses_every_nibble

pytestmark = pytest.mark.gpu

GPU = "cuda:0"
TAPS = 701


def report(name, value):
    print(f"\nresample_stage_errors: {name} = {value:.3e}")


def dev(x):
    return torch.from_numpy(np.array(x, copy=True)).to(GPU)


def interleave(i, q):
    return np.stack([i, q], axis=1).reshape(-1)


def plan_of(s):
    """(fs', the library's own taps, N' = the samples the search needs) of settings with the branch on."""
    new_fs, new_if, wp = native.resample_plan(s)
    eff = s.copy(samplingFreq=new_fs, IF=new_if)
    spc = spc_of(eff)
    need = 2 * spc if s.signal.upper() == "B2A" else int(np.floor(spc / 10 * (10 + s.acqCohT) + 0.5))
    return new_fs, native.fir1_bandpass(TAPS, *wp), need


@functools.lru_cache(maxsize=None)
def b2a():
    s = bds_amd.init_settings_b2a(acqSatelliteList=[19], resamplingflag=1)
    new_fs, b, need = plan_of(s)
    assert (new_fs, need) == (48.06e6, 96120)
    return s, new_fs, b, rc.shortest_input(need, new_fs, s.samplingFreq)


@functools.lru_cache(maxsize=None)
def stream(seed, n, sigma=30.0):
    x = np.clip(np.round(sigma * np.random.default_rng(seed).standard_normal(n)), -128, 127).astype(np.int8)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(key):
    """key -> FiltRef of one real stream; computed once."""
    s, new_fs, b, n = b2a()
    if key in ("I", "Q"):
        return rc.filtfilt_ref(stream({"I": 41, "Q": 42}[key], n), b, new_fs, s.samplingFreq)
    if key in ("packed I", "packed Q"):
        return rc.filtfilt_ref(packed_record()[1][(0 if key == "packed I" else 1)::2], b, new_fs, s.samplingFreq)
    if key == "int16":
        return rc.filtfilt_ref(full_range16(), b, new_fs, s.samplingFreq)
    raise KeyError(key)


@functools.lru_cache(maxsize=None)
def packed_record():
    """(packed bytes, the int8 pairs they unpack to) of n + 1 samples (a byte holds two: the shortest accepted EVEN count)."""
    n = b2a()[3] + 1
    pairs = quantise(interleave(stream(43, n, 20.0), stream(44, n, 20.0)))
    packed = pack_iq(pairs)
    assert uses_every_nibble(packed) and pairs.size == 2 * n
    return packed, pairs


@functools.lru_cache(maxsize=None)
def full_range16():
    n = b2a()[3]
    x = np.random.default_rng(45).integers(-32767, 32768, n).astype(np.int16)
    x[[0, 1, n - 2, n - 1]] = [32767, -32767, 32767, -32767]  # the reflections at both ends reach three times the range
    x.setflags(write=False)
    return x


def block_of(ctx, s, x, is_complex, cap):
    ctx.acq_load(s, x, is_complex)
    return ctx.acq_block(cap)


def within(got, ref):
    assert got.dtype == np.float64 and got.shape == ref.ref.shape
    return rc.worst_ratio(got, ref.ref, ref.tol)


def test_one_stream_five_forms(ctx):
    """One I stream (and one Q stream) as an int8 real record, an int8 I/Q record, the same values as int16 (real and I/Q), and the same
    bytes from device memory (bds_acq_load_dev): every sample within tol2, and all forms bit-equal wherever they hold the same values."""
    s, new_fs, b, n = b2a()
    xi, xq = stream(41, n), stream(42, n)
    s2, s16 = s.copy(fileType=2), s.copy(dataType="int16")
    m = rc.sig_len_of(n, new_fs, s.samplingFreq)
    assert m == 96120 and n == 198751
    real8 = block_of(ctx, s, xi, 0, m)
    iq8 = block_of(ctx, s2, interleave(xi, xq), 1, m)
    real16 = block_of(ctx, s16, xi.astype(np.int16), 0, m)
    iq16 = block_of(ctx, s16.copy(fileType=2), interleave(xi, xq).astype(np.int16), 1, m)
    real8_dev = block_of(ctx, s, dev(xi), 0, m)
    iq8_dev = block_of(ctx, s2, dev(interleave(xi, xq)), 1, m)
    iq16_dev = block_of(ctx, s16.copy(fileType=2), dev(interleave(xi, xq).astype(np.int16)), 1, m)
    assert len(real8) == m and not np.iscomplexobj(real8) and np.iscomplexobj(iq8)
    worst = max(within(real8, reference("I")), within(np.ascontiguousarray(iq8.real), reference("I")), within(np.ascontiguousarray(iq8.imag), reference("Q")))
    report("B2a 99.375 -> 48.06 MS/s, 198 751 samples, int8 real and I/Q: largest error / tol2", worst)
    for name, other in (("int16 real", real16), ("int8 real from device memory", real8_dev), ("I of int8 I/Q", iq8.real)):
        assert rc.same_bits(other, real8), name
    for name, other in (("int16 I/Q", iq16), ("int8 I/Q from device memory", iq8_dev), ("int16 I/Q from device memory", iq16_dev)):
        assert rc.same_bits(other.real, iq8.real) and rc.same_bits(other.imag, iq8.imag), name
    # the block one sample shorter is refused: this one is the shortest accepted
    with pytest.raises(native.BdsError, match="after resampling"):
        ctx.acq_load(s, xi[:-1], 0)


def test_packed_record_with_resampling(ctx):
    """is_complex = 2 with the branch on: unpacked on the device, then conditioned as int8 pairs -- bit-equal to the I/Q record of the
    pairs bds_unpack_cplx makes of the bytes, and within tol2."""
    s, new_fs, b, _ = b2a()
    packed, pairs = packed_record()
    n = pairs.size // 2
    assert np.array_equal(ctx.unpack_cplx(packed), pairs)
    m = rc.sig_len_of(n, new_fs, s.samplingFreq)
    got = block_of(ctx, s.copy(fileType=3), packed, 2, m)
    want = block_of(ctx, s.copy(fileType=2), ctx.unpack_cplx(packed), 1, m)
    assert len(got) == m and rc.same_bits(got.real, want.real) and rc.same_bits(got.imag, want.imag)
    worst = max(within(np.ascontiguousarray(got.real), reference("packed I")), within(np.ascontiguousarray(got.imag), reference("packed Q")))
    report("B2a packed 2+2-bit I/Q, 198 752 samples: largest error / tol2", worst)


def test_full_range_int16(ctx):
    s, new_fs, b, n = b2a()
    x = full_range16()
    assert x.max() == 32767 and x.min() == -32767
    got = block_of(ctx, s.copy(dataType="int16"), x, 0, rc.sig_len_of(n, new_fs, s.samplingFreq))
    report("B2a full-range int16, 198 751 samples: largest error / tol2", within(got, reference("int16")))


@functools.lru_cache(maxsize=None)
def b1c():
    s, x, _ = resample_b1c()
    new_fs, b, need = plan_of(s)
    assert (s.samplingFreq, new_fs, need) == (40e6, 29e6, 580000)
    n = rc.shortest_input(need, new_fs, s.samplingFreq)
    x = np.ascontiguousarray(x[:n])
    x.setflags(write=False)
    return s, new_fs, x, rc.filtfilt_ref(x, b, new_fs, s.samplingFreq)


def test_b1c_40_to_29_on_the_shortest_accepted_block(ctx):
    """helpers.resample_b1c's settings, real record: the rate pair on which float64's ceil((k / fs') fs) differs from the exact ceiling
    most often, on the real path."""
    s, new_fs, x, ref = b1c()
    n = len(x)
    assert 800001 <= n <= 800003
    others = rc.other_orders(len(ref.idx), new_fs, s.samplingFreq)
    assert all(np.any(v != ref.idx) for v in others.values()) and ref.idx.max() <= n
    got = block_of(ctx, s, x, 0, len(ref.ref) + 8)
    assert len(got) == int(np.floor((n - 1) / s.samplingFreq * new_fs)) == len(ref.ref)
    report("B1C 40 -> 29 MS/s, 800 001 samples: largest error / tol2", within(got, ref))
    with pytest.raises(native.BdsError, match="after resampling"):
        ctx.acq_load(s, x[:-1], 0)


def test_acq_block_refusals(ctx):
    """BDS_ERR_ARG, and nothing written: an int8 block, too small a capacity, nothing loaded."""
    s, new_fs, b, n = b2a()
    xi = stream(41, n)
    ctx.acq_load(s, xi, 0)
    m = rc.sig_len_of(n, new_fs, s.samplingFreq)
    re, im, cnt = np.full(m, -7.0), np.full(m, -7.0), native.C.c_longlong(-5)
    lib, dp = ctx._lib, native._DP
    assert lib.bds_acq_block(ctx._h, re.ctypes.data_as(dp), im.ctypes.data_as(dp), m - 1, native.C.byref(cnt)) == -1
    assert np.all(re == -7.0) and np.all(im == -7.0) and cnt.value == -5
    assert lib.bds_acq_block(ctx._h, re.ctypes.data_as(dp), None, m, native.C.byref(cnt)) == 0 and cnt.value == m  # im may be NULL for a real block
    assert rc.same_bits(re, ctx.acq_block(m))
    ctx.acq_load(s.copy(resamplingflag=0), xi, 0)  # an int8 block: there is no float64 block
    re[:] = -7.0
    cnt.value = -5
    assert lib.bds_acq_block(ctx._h, re.ctypes.data_as(dp), im.ctypes.data_as(dp), m, native.C.byref(cnt)) == -1
    assert np.all(re == -7.0) and cnt.value == -5
    with pytest.raises(native.BdsError, match="int8"):
        ctx.acq_block(m)
    with native.Context(0) as fresh:  # nothing loaded
        assert lib.bds_acq_block(fresh._h, re.ctypes.data_as(dp), im.ctypes.data_as(dp), m, native.C.byref(cnt)) == -1
        assert np.all(re == -7.0) and cnt.value == -5
