"""probe_data on the CPU: the float64 restatements of tests/probedata_cases.py against scipy.signal.welch and numpy.histogram, the
derived tolerance against a complex64 model of the kernel's factorisation, the variants the assertion functions must reject, and
the host arithmetic of csrc/bds_probe_math.h built stand-alone under AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.fft
import scipy.signal

import probedata_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FS = 99.375e6


# ---- the restatements ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("n", [32768, 63487, 63488, pc.L5])
def test_welch_model_equals_scipy(cplx, n):
    """to 1e-12 of the largest bin (a bin far below the largest is a difference of rounding errors in either implementation)"""
    x = pc.quantise("s16c" if cplx else "s16", pc.tone_plus_noise(n, cplx, -1234.5 if cplx else 777, seed=n))
    f, want = scipy.signal.welch(x, FS, window=scipy.signal.windows.hamming(32768, sym=True), noverlap=2048, nfft=32768, detrend=False,
                                 scaling="density", return_onesided=not cplx)
    got = pc.welch_model(x, FS)
    assert got.shape == want.shape == ((32768,) if cplx else (16385,))
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(want)
    assert np.allclose(pc.window(), scipy.signal.windows.hamming(32768, sym=True), rtol=0, atol=1e-14)
    assert pc.n_segments(n) == {32768: 1, 63487: 1, 63488: 2, pc.L5: 5}[n]
    np.testing.assert_allclose(f[:3], np.arange(3) * FS / 32768, rtol=1e-15)


def test_hist_model_equals_numpy_histogram():
    rng = np.random.default_rng(5)
    v = np.concatenate([rng.integers(-32768, 32768, 5000), [-32768, 32767, -129, 129, -128, 128, 127, 0], rng.integers(-140, 141, 5000)])
    edges = np.concatenate([[-np.inf], np.arange(-127.5, 128.0, 1.0), [np.inf]])
    want, _ = np.histogram(v, bins=edges)
    got = pc.hist_model(v)
    assert got.shape == (257,) and np.array_equal(got, want) and got.sum() == v.size
    assert got[0] == np.count_nonzero(v <= -128) and got[256] == np.count_nonzero(v >= 128)


def test_bound_constant_is_the_sum_of_the_listed_roundings():
    assert abs(pc.PATH_ROUNDINGS - (2 + (np.sqrt(5) + 1) + 7 + 12 * (np.sqrt(5) + 2) + 1)) < 1e-12
    assert 773.0 < pc.C_BOUND < 773.6 and pc.GAMMA == pc.C_BOUND * 15 * 2.0 ** -24


# ---- a complex64 model of the kernel's factorisation stays inside the bound --------------------------------------------------------
def kernel_model32(x, fs):
    """k_probe_segment in NumPy / scipy.fft single precision: fp32 window and tables, the k1-th output of the 8-point stage with the
    merged twiddle exp(-2 pi i n k1 / 32768) summed over n1 in order, a complex64 4096-point transform, |X|^2 in fp32, then the f64
    sum over the segments in order."""
    x = np.asarray(x)
    cplx = np.iscomplexobj(x)
    w32 = pc.window().astype(np.float32)
    m = np.arange(pc.NFFT)
    tw = (np.cos(-2 * np.pi * m / pc.NFFT).astype(np.float32) + 1j * np.sin(-2 * np.pi * m / pc.NFFT).astype(np.float32)).astype(np.complex64)
    k_seg = pc.n_segments(x.size)
    acc = np.zeros(pc.NFFT)
    n = np.arange(pc.NFFT).reshape(8, 4096)
    for s in range(k_seg):
        seg = x[s * pc.HOP:s * pc.HOP + pc.NFFT]
        v = (w32 * np.real(seg).astype(np.float32) + 1j * (w32 * np.imag(seg).astype(np.float32))).astype(np.complex64).reshape(8, 4096)
        power = np.empty(pc.NFFT, dtype=np.float32)
        for k1 in range(8):
            y = np.zeros(4096, dtype=np.complex64)
            for n1 in range(8):
                y = (y + v[n1] * tw[(n[n1] * k1) % pc.NFFT]).astype(np.complex64)
            z = scipy.fft.fft(y)
            assert z.dtype == np.complex64
            power[k1::8] = z.real * z.real + z.imag * z.imag
        acc += power.astype(np.float64)
    return pc.finish(acc / k_seg, fs, not cplx)


CASES32 = [("noise_real", lambda: pc.quantise("s8", pc.noise(63488, False, 1))),
           ("tone_centre_real", lambda: pc.quantise("s16", pc.tone_plus_noise(63488, False, 3000, 2))),
           ("tone_between_iq", lambda: pc.quantise("s16c", pc.tone_plus_noise(63488, True, -5000.5, 3))),
           ("const127", lambda: np.full(32768, 127.0)),
           ("alternating", lambda: np.where(np.arange(32768) % 2 == 0, 127.0, -128.0)),
           ("stepped_power_iq", lambda: pc.quantise("s16c", 100 * pc.stepped_power(pc.L5, True, 4)))]


@pytest.mark.parametrize("name,make", CASES32)
def test_complex64_model_of_the_factorisation_is_inside_the_bound(name, make):
    x = make()
    pc.assert_psd(kernel_model32(x, FS), x, FS, f"cpu_complex64_model[{name}]")


def test_zero_record_has_zero_bound():
    x = np.zeros(32768)
    assert not pc.welch_bound(x, FS).any() and pc.psd_error_ratio(np.zeros(16385), x, FS) == 0.0
    assert pc.psd_error_ratio(np.full(16385, 1e-300), x, FS) > 1.0


# ---- variants with one change each are rejected by the same assertion functions ----------------------------------------------------
def _welch_variant(x, fs, hop=pc.HOP, window_roll=0, k_div=0, sum_w2=None, double_all=False, double_none=False, conj=False):
    x = np.asarray(x)
    cplx = np.iscomplexobj(x)
    s = pc.segment_spectra(x.astype(np.complex128 if cplx else np.float64), hop=hop, window_roll=window_roll)
    p = np.sum(np.abs(s) ** 2, axis=0) / (s.shape[0] + k_div)
    if conj:
        p = p[(-np.arange(pc.NFFT)) % pc.NFFT]
    out = pc.finish(p, fs, not cplx, sum_w2=sum_w2)
    if double_all:
        out[0] *= 2.0
        out[-1] *= 2.0
    if double_none:
        out[1:-1] /= 2.0
    return out


VARIANTS = {
    "overlap_2047": dict(hop=pc.HOP + 1),
    "window_at_wrong_offset": dict(window_roll=pc.HOP),  # the window indexed from the record's start, not the segment's
    "mean_over_K_plus_1": dict(k_div=1),
    "sum_w_squared": dict(sum_w2=np.sum(pc.window()) ** 2),
    "dc_nyquist_doubled": dict(double_all=True),
    "onesided_not_doubled": dict(double_none=True),
    "conjugated": dict(conj=True),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_changed_welch_models_are_rejected(variant):
    cplx = variant == "conjugated"
    x = pc.quantise("s8c" if cplx else "s8", pc.noise(63489, cplx, 11))  # (two segments also at a hop of 30721)
    assert pc.psd_error_ratio(_welch_variant(x, FS), x, FS) <= 1e-6  # the unchanged variant function is the model
    got = _welch_variant(x, FS, **VARIANTS[variant])
    assert pc.psd_error_ratio(got, x, FS) > 1.0
    with pytest.raises(AssertionError):
        pc.assert_psd(got, x, FS, variant)


def test_exchanged_i_and_q_are_rejected():
    x = pc.quantise("s8c", pc.noise(63488, True, 12) * (1.0 + 0.0j)) * 1.0
    x = np.real(x) + 2j * np.round(np.imag(x) / 2)  # I and Q differently distributed
    sw = np.imag(x) + 1j * np.real(x)
    with pytest.raises(AssertionError):
        pc.assert_psd(pc.welch_model(sw, FS), x, FS, "iq_exchanged")
    st = {f"{k}_{c}": v for c, part in (("i", np.real(x)), ("q", np.imag(x))) for k, v in pc.stats_model(part).items()}
    pc.assert_hist(pc.hist_model(np.real(x)), pc.hist_model(np.imag(x)), st, x, "as_is")
    with pytest.raises(AssertionError):
        pc.assert_hist(pc.hist_model(np.imag(x)), pc.hist_model(np.real(x)), st, x, "iq_exchanged")


def test_hist_that_drops_out_of_range_values_is_rejected():
    v = np.array([-32768, -129, -128, 0, 5, 127, 128, 129, 32767] * 3, dtype=np.float64)
    st = {f"{k}_i": val for k, val in pc.stats_model(v).items()}
    pc.assert_hist(pc.hist_model(v), None, st, v, "clamped")
    inside = v[np.abs(v) <= 128]
    dropped = np.bincount(inside.astype(np.int64) + 128, minlength=257)
    with pytest.raises(AssertionError):
        pc.assert_hist(dropped, None, st, v, "dropped")


# ---- encoders used by the GPU tests ------------------------------------------------------------------------------------------------
def test_encode_round_trips():
    rng = np.random.default_rng(2)
    z = rng.choice([-3, -1, 1, 3], 101) + 1j * rng.choice([-3, -1, 1, 3], 101)
    for lead in (0, 1, 2):
        b = pc.encode("packed", z, lead)
        nib = np.stack([b & 15, b >> 4], axis=1).reshape(-1)[lead:lead + z.size]
        i = np.where(nib & 4, 3, 1) * np.where(nib & 1, -1, 1)
        q = np.where(nib & 8, 3, 1) * np.where(nib & 2, -1, 1)
        assert np.array_equal(i + 1j * q, z)
    v = rng.integers(-32768, 32768, 50)
    assert np.array_equal(pc.encode("s16", v, 3).view("<i2")[3:], v)
    assert np.array_equal(pc.encode("s8c", v[:10] % 100 + 1j * (v[10:20] % 50), 1).view(np.int8)[2::2], v[:10] % 100)


# ---- the host arithmetic of the library, stand-alone under the sanitizers ----------------------------------------------------------
def _pieces(n, spp):
    k = pc.n_segments(n)
    out = []
    for j in range(-(-k // spp)):
        s0, s1 = j * spp, min((j + 1) * spp, k)
        last = s1 == k
        out.append((s0, s1, s0 * pc.HOP, n if last else s1 * pc.HOP, s0 * pc.HOP, n if last else (s1 - 1) * pc.HOP + pc.NFFT))
    return k, out


def test_host_arithmetic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "probe_math_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "bds-3-b1c-b2a-sdr-receiver_amd", "csrc"),
                           os.path.join(HERE, "host_models", "probe_math_check.cpp"), "-o", exe])
    bits = [8, 16, 4, 16, 32]
    pcs = [(f, n, spp) for f in range(5) for n in (32767, 32768, 63487, 63488, pc.L5, 10 ** 6 + 1) for spp in (1, 2, 3, 1000)] + [(0, 3 * 10 ** 9, 0), (2, 3 * 10 ** 9, 0)]
    args = [(0, 32768, 10, 16385, 0, 1, 0, 32768), (0, 32767, 0, 16385, 0, 1, -1, -1), (0, 32768, 0, 16384, 0, 1, -1, -1), (1, 65537, 0, 32768, 1, 1, -1, -1),
            (1, 65536, 0, 32768, 1, 1, 0, 32768), (1, 65536, 0, 32768, 0, 1, -1, -1), (2, 16384, 0, 32768, 1, 1, 0, 32768), (3, 65537, 0, 16385, 0, 1, -1, -1),
            (4, 131074, 0, 32768, 1, 1, -1, -1), (4, 131072, 5, 32768, 1, 0, -1, -1), (4, 131072, 32769, 32768, 1, 1, -1, -1), (4, 131072, 32768, 32768, 1, 1, 0, 32768)]
    lines = [f"P {f} {n} {spp}" for f, n, spp in pcs] + [f"A {a[0]} {a[1]} {a[2]} {a[3]} {a[4]} {a[5]}" for a in args] + ["F 0"]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.check_output([exe], input="\n".join(lines).encode(), timeout=120, env=env).decode().strip().split("\n")
    w = pc.window()
    got = [float(v) for v in out[0].split()[1:]]
    assert abs(got[0] - np.sum(w * w)) <= 1e-12 * got[0]
    assert got[1:] == [float(np.float32(w[i])) for i in (0, 1, 16383, 32767)]
    for line, m in zip(out[1:4], (1, 8192, 32767)):
        re_, im_ = (float(v) for v in line.split()[1:])
        assert abs(re_ - np.cos(2 * np.pi * m / 32768)) <= 2.0 ** -24 and abs(im_ + np.sin(2 * np.pi * m / 32768)) <= 2.0 ** -24
    i = 4
    for f, n, spp in pcs:
        if spp == 0:
            spp = ((256 << 20) * 8 // bits[f] - 2048) // 30720
        k, want = _pieces(n, spp)
        assert out[i] == f"P {k} {len(want)}", (f, n, spp)
        i += 1
        covered = 0
        for p in want:
            b0, b1 = p[4] * bits[f] // 8, (p[5] * bits[f] + 7) // 8
            assert out[i] == "p " + " ".join(str(v) for v in p + (b0, b1)), (f, n, spp)
            assert p[2] == covered and p[5] <= n and p[0] * pc.HOP >= p[4] and (p[1] - 1) * pc.HOP + pc.NFFT <= p[5]
            covered = p[3]
            i += 1
        assert covered == (n if k else 0)
    for a in args:
        rc, n = out[i].split()[1:3]
        assert (int(rc), int(n)) == (a[6], a[7]), (a, out[i])
        assert int(rc) == 0 or len(out[i].split()) > 3  # an error carries its message
        i += 1
    f0 = [float(v) for v in out[i].split()[2:]]
    f1 = [float(v) for v in out[i + 1].split()[2:]]
    sc = 1.0 / (2.0 * 8.0)
    assert f0 == [1 / 4 * sc, 2 * (2 / 4 * sc), 16385 / 4 * sc, 16385 / 4 * sc] and f1 == [1 / 4 * sc, 2 / 4 * sc, 16385 / 4 * sc, 32768 / 4 * sc]


# ---- the public surface (fails on a tree without the feature) --------------------------------------------------------------------------
def test_entries_are_declared_bound_and_documented():
    import bds_amd
    from bds_amd import native

    src = open(os.path.join(ROOT, "include", "bds_mi355x.h")).read()
    for entry in ("bds_probe_data", "bds_probe_data_file", "bds_probe_set_piece_segments"):
        assert re.search(r"BDS_API\s+int\s+%s\s*\(" % entry, src) and entry in native.EXPORTS
    assert re.search(r"BDS_PROBE_DEV_API\s+int\s+bds_probe_data_dev\s*\(", src) and native.PROBE_DEVICE_EXPORTS == ["bds_probe_data_dev"]
    assert "typedef struct bds_probe_out" in src and "probeData.m:76" in src and "probeData.m:128" in src
    assert callable(bds_amd.probe_data) and callable(native.Context.probe_data)
    import ctypes

    built = ctypes.CDLL(native._LIB_PATH)  # (symbols only)
    for entry in native.PROBE_DEVICE_EXPORTS + ["bds_probe_data", "bds_probe_data_file", "bds_probe_set_piece_segments"]:
        assert hasattr(built, entry), entry
    s = bds_amd.init_settings_b2a()
    from bds_amd import probedata

    assert probedata.samples_per_code(s) == 99375 and probedata.excerpt_length(s) == 199
    assert probedata.excerpt_length(bds_amd.init_settings_b2a(fileType=2)) == 49688
    with pytest.raises(TypeError, match="Incorect number of arguments"):
        bds_amd.probe_data()
