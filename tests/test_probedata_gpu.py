"""probe_data on the GPU (csrc/bds_probedata.hip) against the float64 restatements of tests/probedata_cases.py: the histogram and the
integer statistics exactly, the PSD within the tolerance derived there (each test prints its worst |error| / bound; the values
measured on an MI355X are in profiles/probedata_errors.txt), the excerpt exactly -- for the five record formats, from host memory,
from a file behind an odd skipNumberOfBytes, from a device pointer one element past its allocation, and from a file forced into
pieces of two segments, all four bit for bit alike."""
import ctypes

import numpy as np
import pytest
import torch

import bds_amd
from bds_amd import native
from bds_amd.synth import Sat, make_if_device

import probedata_cases as pc

pytestmark = pytest.mark.gpu
FS = 99.375e6
SKIP = 3  # samples of filler in front of a file's window: odd, so a packed window starts at a high nibble


def settings_of(fmt, **over):
    file_type, data_type = pc.FORMAT_SETTINGS[fmt]
    return bds_amd.init_settings_b2a(fileType=file_type, dataType=data_type, samplingFreq=FS, **over)


def as_record(fmt, raw):
    """The bytes as the array type the format's records are passed as (int16 samples for the 16-bit formats)."""
    return raw.view("<i2") if fmt in ("s16", "s16c") else raw if fmt == "packed" else raw.view(np.int8)


def device_record(fmt, x):
    """The record in device memory, one element past the start of its allocation."""
    a = as_record(fmt, pc.encode(fmt, x))
    t = torch.from_numpy(np.concatenate([np.full(1, 0x5A, dtype=a.dtype), a])).to("cuda:0")
    return t[1:]


def fields(r):
    return dict(hist_i=r.hist_i, hist_q=r.hist_q, psd=r.psd, excerpt=r.excerpt, n_segments=r.n_segments, n_samples=r.n_samples,
                sums=sorted(r.sums.items()))


def assert_same(a, b, what):
    fa, fb = fields(a), fields(b)
    for k in fa:
        if isinstance(fa[k], np.ndarray):
            assert fa[k].dtype == fb[k].dtype and np.array_equal(fa[k].view(np.uint8), fb[k].view(np.uint8)), (what, k)
        else:
            assert fa[k] == fb[k], (what, k)


def probe_every_source(fmt, x, tmp_path, ctx, n_time=37):
    """probe_data of x from host memory, a device pointer, a file and the file and the host memory cut into pieces of two
    segments; asserts that they agree bit for bit and returns one result.  A packed array holds whole bytes, so an odd number of
    packed samples exists only as a file window: the arrays then hold one sample more (the pad nibble 0 = +1 + 1j), are held
    against the model of that record here, and the file's result is returned."""
    x = np.asarray(x)
    s = settings_of(fmt)
    odd_packed = fmt == "packed" and x.size % 2 == 1
    x_mem = np.concatenate([x, [1 + 1j]]) if odd_packed else x
    host = bds_amd.probe_data(as_record(fmt, pc.encode(fmt, x_mem)), s, n_time=n_time)
    dev = bds_amd.probe_data(device_record(fmt, x_mem), s, n_time=n_time)
    assert_same(host, dev, "device pointer")
    path = str(tmp_path / f"rec_{fmt}_{x.size}.bin")
    np.concatenate([pc.encode(fmt, x, lead=SKIP), np.full(9, 0xC3, dtype=np.uint8)]).tofile(path)  # (the tail is not in the window)
    sf = settings_of(fmt, skipNumberOfBytes=SKIP)
    file = bds_amd.probe_data(path, sf, n_samples=x.size, n_time=n_time)
    ctx.probe_set_piece_segments(2)
    try:
        assert_same(file, bds_amd.probe_data(path, sf, n_samples=x.size, n_time=n_time), "file in pieces of 2 segments")
        assert_same(host, bds_amd.probe_data(as_record(fmt, pc.encode(fmt, x_mem)), s, n_time=n_time), "host memory in pieces of 2 segments")
    finally:
        ctx.probe_set_piece_segments(0)
    if odd_packed:
        check(host, x_mem, f"packed[{x_mem.size}, arrays]")
    else:
        assert_same(host, file, "file")
    return file


def check(r, x, name):
    """every output of one result against the model of the same samples"""
    x = np.asarray(x)
    cplx = np.iscomplexobj(x)
    assert r.n_samples == x.size and r.n_segments == pc.n_segments(x.size)
    assert r.psd.shape == ((32768,) if cplx else (16385,)) and np.array_equal(r.freq, np.arange(r.psd.size) * (FS / 32768))
    pc.assert_hist(r.hist_i, r.hist_q, r.sums, x, name)
    assert np.array_equal(r.excerpt, x[:r.excerpt.size]) and r.excerpt.dtype == (np.complex128 if cplx else np.float64)
    parts = [np.real(x), np.imag(x)] if cplx else [x]
    for got, want in ((r.mean, [p.sum() / x.size for p in parts]), (r.rms, [np.sqrt(np.sum(p.astype(np.float64) ** 2) / x.size) for p in parts]),
                      (r.min, [p.min() for p in parts]), (r.max, [p.max() for p in parts])):
        np.testing.assert_allclose(np.atleast_1d(got), want, rtol=1e-15)
    return pc.assert_psd(r.psd, x, FS, name)


# ---- formats x lengths x sources ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", pc.LENGTHS)
@pytest.mark.parametrize("fmt", pc.FORMATS)
def test_formats_lengths_and_sources(ctx, tmp_path, fmt, n):
    cplx = pc.is_complex(fmt)
    x = pc.quantise(fmt, pc.tone_plus_noise(n, cplx, -4100.5 if cplx else 4100.5, seed=n % 1000 + len(fmt)))
    r = probe_every_source(fmt, x, tmp_path, ctx)
    assert r.excerpt.size == 37
    check(r, x, f"{fmt}[{n}]")


@pytest.mark.parametrize("fmt", pc.FORMATS)
def test_too_short_a_record_is_an_argument_error(ctx, tmp_path, fmt):
    """32767 samples (a packed array holds whole bytes: 32766 there; the file entry takes 32767 of every format)"""
    long = pc.quantise(fmt, pc.noise(40000, pc.is_complex(fmt), 7))
    x = long[:32766 if fmt == "packed" else 32767]
    s = settings_of(fmt)
    path = str(tmp_path / "short.bin")
    pc.encode(fmt, long).tofile(path)
    for source, kw in ((as_record(fmt, pc.encode(fmt, x)), {}), (device_record(fmt, x), {}), (path, dict(n_samples=32767))):
        with pytest.raises(native.BdsError, match="pwelch needs at least one segment") as e:
            bds_amd.probe_data(source, s, n_time=0, **kw)
        assert e.value.code == -1
    with pytest.raises(native.BdsError, match="Could not read enough data") as e:  # probeData.m:81-84
        bds_amd.probe_data(path, s, n_samples=40001, n_time=0)
    assert e.value.code == -1
    assert bds_amd.probe_data(path, s, n_samples=40000, n_time=0).n_samples == 40000
    with pytest.raises(native.BdsError, match="Could not read enough data"):
        bds_amd.probe_data(path, s, n_time=0)  # the reference's window: 5 code periods


def test_odd_byte_counts_and_a_small_psd_array_write_nothing(ctx):
    for fmt, n_bytes in (("s8c", 65537), ("s16", 65537), ("s16c", 131074)):
        raw = np.zeros(n_bytes, dtype=np.uint8)
        cs = native.pack_settings(settings_of(fmt))
        o, keep = _probe_out(32768)
        rc = ctx._lib.bds_probe_data(ctx._h, ctypes.byref(cs), raw.ctypes.data_as(ctypes.c_void_p), raw.size, 0, ctypes.byref(o))
        assert rc == -1 and b"whole number of samples" in ctx._lib.bds_last_error(ctx._h)
        assert all(np.isnan(a).all() if a.dtype == np.float64 else (a == -7).all() for a in keep)
    raw = np.zeros(32768, dtype=np.uint8)
    cs = native.pack_settings(settings_of("s8"))
    o, keep = _probe_out(16384)
    rc = ctx._lib.bds_probe_data(ctx._h, ctypes.byref(cs), raw.ctypes.data_as(ctypes.c_void_p), raw.size, 0, ctypes.byref(o))
    assert rc == -1 and b"16385" in ctx._lib.bds_last_error(ctx._h)
    assert all(np.isnan(a).all() if a.dtype == np.float64 else (a == -7).all() for a in keep) and o.n_psd == -7 and o.n_segments == -7
    with pytest.raises(native.BdsError, match="fileType 3"):
        bds_amd.probe_data(np.zeros(40000, dtype=np.int16), bds_amd.init_settings_b2a(fileType=3, dataType="int16"), n_time=0)


def _probe_out(cap):
    hi, hq, psd = np.full(257, -7, dtype=np.int64), np.full(257, -7, dtype=np.int64), np.full(cap, np.nan)
    o = native.ProbeOut()
    i64 = ctypes.POINTER(ctypes.c_int64)
    o.hist_i, o.hist_q, o.psd, o.cap = hi.ctypes.data_as(i64), hq.ctypes.data_as(i64), psd.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), cap
    o.n_psd, o.n_segments = -7, -7
    return o, (hi, hq, psd)


# ---- histogram: exact --------------------------------------------------------------------------------------------------------------------
N_H = 32768 + 1234 + 7  # one segment, and a tail whose head and tail bytes leave the 16-byte lines ragged


def _hist_cases():
    rng = np.random.default_rng(21)
    t = np.arange(N_H)
    yield "s8", "constant", np.full(N_H, -5.0)
    yield "s8", "only_-128_and_127", np.where(rng.random(N_H) < 0.3, -128.0, 127.0)
    yield "s16", "end_bins", rng.choice([129, -129, 32767, -32767, -32768, 128, -128, 127, 0], N_H).astype(np.float64)
    yield "s16", "constant_-32768", np.full(N_H, -32768.0)
    yield "s16c", "end_bins_iq", rng.choice([129, 32767, 5], N_H) + 1j * rng.choice([-129, -32768, -32767, -5, 0], N_H)
    yield "s8c", "i_ne_q", rng.integers(-128, 20, N_H) + 1j * rng.integers(-3, 128, N_H)
    yield "packed", "four_levels", rng.choice([-3, -1, 1, 3], N_H, p=[0.1, 0.2, 0.3, 0.4]) + 1j * rng.choice([-3, -1, 1, 3], N_H, p=[0.4, 0.3, 0.2, 0.1])
    yield "packed", "one_level", np.full(N_H, -3.0 + 1.0j)
    yield "s8c", "constant_iq", np.where(t >= 0, 127.0 - 128.0j, 0)


@pytest.mark.parametrize("fmt,name,x", [pytest.param(f, n, x, id=f"{f}-{n}") for f, n, x in _hist_cases()])
def test_histogram_and_statistics_are_exact(ctx, tmp_path, fmt, name, x):
    r = probe_every_source(fmt, x, tmp_path, ctx, n_time=5)
    pc.assert_hist(r.hist_i, r.hist_q, r.sums, x, name)
    assert int(r.hist_i.sum()) == N_H and (r.hist_q is None or int(r.hist_q.sum()) == N_H)
    if name == "constant":
        assert r.hist_i[123] == N_H and np.count_nonzero(r.hist_i) == 1
    if name == "constant_-32768":
        assert r.hist_i[0] == N_H and r.sums["sumsq_i"] == N_H * 32768 ** 2 and r.min == r.max == -32768
    if name == "i_ne_q":
        assert not np.array_equal(r.hist_i, r.hist_q)


# ---- PSD: within the derived bound ---------------------------------------------------------------------------------------------------------
def test_zero_record_gives_exactly_zero(ctx):
    for fmt in ("s8", "s16c"):
        x = np.zeros(63488, dtype=np.complex128 if pc.is_complex(fmt) else np.float64)
        r = bds_amd.probe_data(device_record(fmt, x), settings_of(fmt), n_time=0)
        assert not r.psd.any() and r.hist_i[128] == 63488 and r.n_segments == 2


def test_constant_and_alternating_records(ctx):
    s = settings_of("s8")
    c = np.full(63488, 127.0)
    r = bds_amd.probe_data(device_record("s8", c), s, n_time=0)
    check(r, c, "constant_127")  # (the bins far from DC hold the Hamming side lobes and below: the absolute term of the bound)
    assert np.argmax(r.psd) == 0
    a = np.where(np.arange(63488) % 2 == 0, 127.0, -128.0)
    r = bds_amd.probe_data(device_record("s8", a), s, n_time=0)
    check(r, a, "alternating_127_-128")
    assert np.argmax(r.psd) == 16384
    z = np.full(63488, 127.0 - 128.0j)
    r = bds_amd.probe_data(device_record("s16c", z), settings_of("s16c"), n_time=0)
    check(r, z, "constant_iq_int16")


@pytest.mark.parametrize("fmt", ["s8", "s16", "packed", "s8c", "s16c"])
@pytest.mark.parametrize("where", ["centre", "between"])
def test_tone_60_db_above_the_noise(ctx, fmt, where):
    """sigma = 20 noise plus a tone 60 dB above it, at a bin centre and halfway between two bins; of an I/Q record at a NEGATIVE
    frequency: the peak is at bin 32768 - k, not k."""
    cplx = pc.is_complex(fmt)
    k = 3000 + (0.5 if where == "between" else 0.0)
    x = pc.quantise(fmt, pc.tone_plus_noise(63488, cplx, -k if cplx else k, seed=31))
    r = bds_amd.probe_data(device_record(fmt, x), settings_of(fmt), n_time=0)
    check(r, x, f"tone_{where}[{fmt}]")
    peak = int(np.argmax(r.psd))
    assert peak in ((32768 - 3000, 32768 - 3001) if cplx else (3000, 3001))
    if fmt in ("s16", "s16c") and where == "centre":
        floor = np.median(r.psd)
        assert 10 * np.log10(r.psd[peak] / floor) > 58  # (the median of a chi-square floor lies 1.6 dB under its mean)


@pytest.mark.parametrize("fmt", ["s16", "s16c", "s8"])
def test_segments_that_differ_by_40_db(ctx, tmp_path, fmt):
    x = pc.quantise(fmt, (100 if fmt != "s8" else 1.2) * pc.stepped_power(pc.L5, pc.is_complex(fmt), 41))
    p = [np.mean(np.abs(x[i * pc.HOP:(i + 1) * pc.HOP]) ** 2) for i in (0, 4)]
    assert fmt == "s8" or 39 < 10 * np.log10(p[1] / p[0]) < 41
    r = probe_every_source(fmt, x, tmp_path, ctx)
    assert r.n_segments == 5
    check(r, x, f"stepped_power[{fmt}]")


# ---- the reference's call forms, and a record that exists only in device memory ------------------------------------------------------------
def test_reference_window_and_whole_file(ctx, tmp_path):
    """probe_data(fileName, settings) and probe_data(settings) read 5 code periods behind skipNumberOfBytes (B2a/include/probeData.m:76),
    10 for B1C (B1C/include/probeData.m:76); n_samples="all" reads to the end of the file."""
    s = bds_amd.init_settings_b2a(fileType=1, dataType="schar", samplingFreq=8.184e6, skipNumberOfBytes=5)
    spc = 8184
    x = pc.quantise("s8", pc.noise(5 + 10 * spc + 100, False, 51))
    path = str(tmp_path / "ref.bin")
    x.astype(np.int8).tofile(path)
    s.fileName = path
    r = bds_amd.probe_data(s)
    assert r.n_samples == 5 * spc and r.excerpt.size == round(spc / 500)
    want = bds_amd.probe_data(x[5:5 + 5 * spc].astype(np.int8), s, n_time=r.excerpt.size)
    assert_same(r, want, "reference window")
    assert_same(bds_amd.probe_data(path, s), r, "two call forms")
    b1c = bds_amd.init_settings_b1c(fileType=1, dataType="schar", samplingFreq=0.8184e6, skipNumberOfBytes=5)  # 8184 samples per 10-ms code
    r = bds_amd.probe_data(path, b1c)
    assert r.n_samples == 10 * spc and r.excerpt.size == spc // 2
    r = bds_amd.probe_data(path, s, n_samples="all")
    assert r.n_samples == x.size - 5
    pc.assert_hist(r.hist_i, None, r.sums, x[5:], "whole file")


def test_device_generated_record_equals_its_download(ctx):
    s = bds_amd.init_settings_b2a(fileType=2, dataType="schar", samplingFreq=FS)
    t = make_if_device(s, [Sat(19, 1200.0, 3000.0, 0.3, 48.0)], 70000, iq_sign=1, out="torch")
    assert t.is_cuda and t.dtype == torch.int8 and t.numel() == 140000
    dev = bds_amd.probe_data(t, s)
    host = bds_amd.probe_data(t.cpu().numpy(), s)
    assert_same(dev, host, "device record")
    v = t.cpu().numpy().astype(np.float64)
    x = v[0::2] + 1j * v[1::2]
    assert dev.excerpt.size == 49688
    check(dev, x, "make_if_device")
