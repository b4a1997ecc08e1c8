"""The tone excisor without a GPU: the vectorised model equals the definition, the library's LO table equals NumPy's, notch_step's
rounding, pieces on the block grid reproduce the whole, the argument refusals of the three entries before any device call, the CW
generator, the detector on PSDs computed here, the refiner on the model's estimates, and the jammed scene on the float64 oracle."""
import ctypes as C
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import bds_amd
from bds_amd import native, synth
from oracle import acquisition as oacq

import notch_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B8 = 256


@pytest.fixture(scope="module")
def scene():
    return nc.cw_scenario()


@pytest.mark.parametrize("fmt", list(nc.FORMATS))
def test_vectorised_model_equals_the_definition(fmt):
    for n in (1, B8 - 1, B8, B8 + 1, 3 * B8 + 37):
        for k in (1, 2, 8):
            steps = nc.steps_for(fmt, 8, k)
            rec = nc.with_tones(fmt, n, steps[:3], seed=n + k)
            for first, apply in ((0, True), (5 * B8, True), (0, False)):
                a, ra = nc.model_definition(rec, fmt, steps, 8, first, apply)
                b, rb = nc.model(rec, fmt, steps, 8, first, apply)
                assert (a is None and b is None) if not apply else np.array_equal(a, b), (n, k, first)
                assert set(ra) == set(rb)
                for key in ra:
                    assert np.array_equal(ra[key], rb[key]), (key, n, k, first)
    # a record the subtraction saturates: a last block of two samples at the minimum is estimated as all tone, and y = -x
    rec = np.concatenate([nc.noise(fmt, B8, seed=1), np.full(2 * nc.FORMATS[fmt][3], np.iinfo(nc.FORMATS[fmt][2]).min, dtype=nc.FORMATS[fmt][2])])
    steps = nc.steps_for(fmt, 8, 1)
    a, ra = nc.model_definition(rec, fmt, steps, 8)
    b, rb = nc.model(rec, fmt, steps, 8)
    assert np.array_equal(a, b) and ra["n_saturated"] == rb["n_saturated"] and ra["sum_sq_out"] == rb["sum_sq_out"]


def test_the_model_removes_the_tone():
    """int8, sigma 6, amplitude 100, B = 1024: the residual against the clean record is quantisation-sized (measured 0.44 LSB rms)"""
    n, st = 64 * 1024, [bds_amd.notch_step(6.9e6, 25e6)]
    clean = nc.noise("s8", n, seed=3)
    jam = np.clip(np.rint(clean + 100.0 * np.cos(2 * np.pi * st[0] / 2 ** 32 * np.arange(n) + 0.7)), -127, 127).astype(np.int8)
    out, rep = nc.model(jam, "s8", st, 10)
    rms = float(np.sqrt(np.mean((out.astype(np.float64) - clean) ** 2)))
    # per block the estimate carries noise of variance 2 (sigma^2 + 1/12) / B in amplitude: 0.27 LSB rms on the subtracted
    # cosine's amplitude, 0.19 on its samples; the two roundings add 1/12 each
    assert rms <= math.sqrt(2 * (36 + 1 / 12) / 1024 + 2 / 12) * 1.5
    assert rep["n_saturated"] == 0 and rep["sum_sq_in"] > 50 * rep["sum_sq_out"] > 0


def test_lo_table_is_numpys_and_symmetric():
    t = native.notch_lo().astype(np.int64)
    n, q = 1 << nc.P, 1 << (nc.P - 2)
    i = np.arange(n)
    np.testing.assert_array_equal(t[0], np.rint(nc.L * np.cos(2 * np.pi * i / n)).astype(np.int64))
    np.testing.assert_array_equal(t[1], np.rint(nc.L * np.sin(2 * np.pi * i / n)).astype(np.int64))
    c, s = nc.lo_table()
    np.testing.assert_array_equal(t[0], c)
    np.testing.assert_array_equal(t[1], s)
    s = t[1]
    np.testing.assert_array_equal(s[(n - i) % n], -s)              # odd
    np.testing.assert_array_equal(s[(2 * q - i) % n], s)           # mirrored about the quarter turn
    np.testing.assert_array_equal(s[(i + 2 * q) % n], -s)          # half a turn on
    np.testing.assert_array_equal(t[0], s[(i + q) % n])            # the cosine is the sine a quarter turn on
    assert s[q] == nc.L and s[0] == 0 and t[0][0] == nc.L and abs(t).max() == nc.L


def test_notch_step_rounds_half_up_and_wraps():
    fs = 25e6
    assert bds_amd.notch_step(0.0, fs) == 0
    assert bds_amd.notch_step(fs / 2 ** 33, fs) == 1          # a tie goes up
    assert bds_amd.notch_step(-fs / 2 ** 33, fs) == 0         # ... also below zero: floor(-0.5 + 0.5)
    assert bds_amd.notch_step(-fs / 2 ** 32, fs) == 2 ** 32 - 1
    assert bds_amd.notch_step(-fs / 4, fs) == 3 << 30
    assert bds_amd.notch_step(fs / 2, fs) == 1 << 31 and bds_amd.notch_step(-fs / 2, fs) == 1 << 31
    assert bds_amd.notch_step(fs, fs) == 0
    assert bds_amd.notch_step(6.5e6, fs) == int(math.floor(6.5e6 / fs * 2 ** 32 + 0.5))


@pytest.mark.parametrize("fmt", list(nc.FORMATS))
def test_pieces_on_the_block_grid_reproduce_the_whole(fmt):
    n = 5 * B8 + 37
    steps = nc.steps_for(fmt, 8, 3)
    rec = nc.with_tones(fmt, n, steps, seed=4)
    whole, rep = nc.model(rec, fmt, steps, 8)
    for piece in (B8, 2 * B8, 8 * B8):
        got, est, tot = nc.pieces(rec, fmt, steps, 8, piece)
        np.testing.assert_array_equal(got, whole)
        np.testing.assert_array_equal(est, rep["est"])
        assert tot == (rep["n_blocks"], rep["n_saturated"], rep["sum_sq_in"], rep["sum_sq_out"])
    with pytest.raises(ValueError, match="off the block grid"):
        nc.pieces(rec, fmt, steps, 8, B8 + 1)
    # a piece that is not told where it starts gets the phases wrong
    c = nc.FORMATS[fmt][3]
    assert not np.array_equal(nc.model(rec[B8 * c:], fmt, steps, 8)[0], whole[B8 * c:])


def _call(entry="bds_notch", fmt="s8", n_bytes=1024, steps=None, beta=8, first=0, apply=1, cap=None, out_shift=None, s=None, piece=0, paths=None):
    lib = native.lib()
    cs = native.pack_settings(s or nc.settings_of(fmt))
    o, rep = native.pack_notch(nc.steps_for(fmt, min(max(beta, 8), 16), 1) if steps is None else steps, beta, first, apply)
    est = np.zeros(64, dtype=np.int32)
    if cap is not None:
        rep.est, rep.est_cap = est.ctypes.data_as(native._IP), cap
    buf = np.zeros(4096, dtype=np.int16)
    p_in = buf.ctypes.data
    p_out = p_in if out_shift is None else p_in + out_shift
    if entry == "bds_notch_file":
        return lib.bds_notch_file(None, C.byref(cs), paths[0], paths[1], -1, piece, C.byref(o), C.byref(rep))
    return getattr(lib, entry)(None, C.byref(cs), C.c_void_p(p_in), n_bytes, C.c_void_p(p_out), C.byref(o), C.byref(rep))


def test_argument_checks_come_before_any_device_call(tmp_path):
    """Every argument error is BDS_ERR_ARG (fileType 3: BDS_ERR_UNSUPPORTED) with a message, raised with no context at all."""
    err = lambda: native.lib().bds_last_error(None).decode()
    w = nc.width(8)
    for entry in ("bds_notch", "bds_notch_dev"):
        assert _call(entry, steps=[]) == -1 and "n_tones = 0" in err()
        assert _call(entry, steps=nc.steps_for("s8c", 8, 8) + [5]) == -1 and "n_tones = 9" in err()
        assert _call(entry, beta=7, steps=[1 << 30]) == -1 and "block_log2 = 7" in err()
        assert _call(entry, beta=17, steps=[1 << 30]) == -1 and "block_log2 = 17" in err()
        assert _call(entry, first=-256) == -1 and "first_sample" in err()
        assert _call(entry, first=255) == -1 and "not on the grid" in err()
        assert _call(entry, fmt="s8c", steps=[5 * w, 9 * w - 1]) == -1 and "closer than four notch widths" in err()
        assert _call(entry, fmt="s8c", steps=[2 * w, 2 ** 32 - 2 * w + 1]) == -1 and "closer than four" in err()  # across the wrap
        assert _call(entry, steps=[2 * w - 1]) == -1 and "image" in err()
        assert _call(entry, steps=[(1 << 31) - 2 * w + 1]) == -1 and "image" in err()
        assert _call(entry, steps=[0]) == -1 and "image" in err()
        assert _call(entry, steps=[(1 << 31) + 5 * w]) == -1 and "image" in err()
        assert _call(entry, fmt="s8c", n_bytes=63) == -1 and "whole number of samples" in err()
        assert _call(entry, fmt="s16", n_bytes=63) == -1 and "whole number of samples" in err()
        assert _call(entry, fmt="s16c", n_bytes=62) == -1 and "whole number of samples" in err()
        assert _call(entry, out_shift=16) == -1 and "overlap" in err()
        assert _call(entry, n_bytes=1025, steps=[8 * w, 20 * w], cap=9) == -1 and "holds 9 estimates, the window takes 10" in err()
        assert _call(entry, s=nc.settings_of("s8").copy(fileType=3)) < -1 and "no amplitude to subtract from" in err()
        # valid arguments get as far as the missing context: the limits themselves are admitted
        assert _call(entry) == -1 and "ctx is NULL" in err()
        assert _call(entry, steps=[2 * w, (1 << 31) - 2 * w, 6 * w], out_shift=2048) == -1 and "ctx is NULL" in err()
        assert _call(entry, fmt="s8c", steps=[0, 4 * w, 2 ** 32 - 4 * w], first=512, cap=12) == -1 and "ctx is NULL" in err()
        assert _call(entry, apply=0, out_shift=16) == -1 and "ctx is NULL" in err()  # (an estimate-only call has no output to overlap)
    assert _call("bds_notch_dev", fmt="s16", out_shift=2049) == -1 and "aligned" in err()
    src, dst = tmp_path / "in.bin", tmp_path / "never_written.bin"
    np.zeros(1000, dtype=np.int8).tofile(src)
    paths = (os.fsencode(src), os.fsencode(dst))
    assert _call("bds_notch_file", paths=paths, piece=255) == -1 and "smaller than one block" in err()
    assert _call("bds_notch_file", paths=paths, piece=-1) == -1 and "piece_samples" in err()
    assert _call("bds_notch_file", paths=paths, steps=[5]) == -1 and "image" in err()
    assert _call("bds_notch_file", paths=paths, cap=3) == -1 and "holds 3 estimates, the window takes 4" in err()
    assert _call("bds_notch_file", paths=(paths[0], paths[0])) == -1 and "same file" in err()
    assert _call("bds_notch_file", paths=paths, s=nc.settings_of("s8", skipNumberOfBytes=1001)) == -1 and "Could not read enough data" in err()
    assert _call("bds_notch_file", paths=paths, s=nc.settings_of("s8").copy(fileType=3)) < -1 and "no amplitude" in err()
    assert _call("bds_notch_file", paths=paths, piece=300, cap=4) == -1 and "ctx is NULL" in err()
    assert not os.path.exists(dst)
    with pytest.raises(ValueError, match="uint32"):
        native.pack_notch([2 ** 32], 8)
    with pytest.raises(ValueError, match="power of two"):
        bds_amd.notch_tones(np.zeros(1024, np.int8), nc.settings_of("s8"), [1e6], block=1000)


def test_host_arithmetic_under_sanitizers(tmp_path):
    """csrc/bds_notch_math.h in a stand-alone program under AddressSanitizer and UBSan, held to Python's integers"""
    import subprocess

    exe = str(tmp_path / "notch_math_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "bds-3-b1c-b2a-sdr-receiver_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_models", "notch_math_check.cpp"), "-o", exe])
    rng = np.random.default_rng(1)
    rs = [1, 2, 3, 255, 256, 257, 1000, 65535, 65536]
    # |sum| <= r 2^30 (an int16 pair's I C + Q S stays below 2^15 2^14 sqrt(2)): 2^46 at r = 65536, and an estimate of at most 2^24
    cases = [(s, r) for r in rs for s in [0, 1, -1, r << 30, -(r << 30), (r << 30) - 1, 1 - (r << 30)] + [int(v) for v in rng.integers(-(r << 30), r << 30, 8)]]
    es = [0, 1, -1, 2 ** 20 - 1, 2 ** 20, -2 ** 20, -2 ** 20 - 1, 2 ** 42, -2 ** 42] + [int(v) for v in rng.integers(-2 ** 42, 2 ** 42, 20)]
    idx = [(0xFFFFFFFF, 2 ** 40 + 3), (1 << 17, 1), ((1 << 17) - 1, 1), (123456789, 987654321), (0x80000000, 1)]
    w = nc.width(8)
    args = [("0 1024 1 8 0 -1 %d" % (2 * w), 0), ("0 1024 1 8 0 -1 %d" % (2 * w - 1), -1), ("1 1024 2 8 256 4 %d %d" % (w // 3, 4 * w + w // 3), 0),
            ("1 1024 2 8 256 3 %d %d" % (w // 3, 4 * w + w // 3), -1), ("1 1024 2 8 256 4 %d %d" % (w // 3, 4 * w + w // 3 - 1), -1), ("4 1022 1 8 0 -1 5", -1),
            ("3 1024 0 8 0 -1", -1), ("3 1024 1 17 0 -1 %d" % (1 << 30), -1), ("3 1024 1 8 100 -1 %d" % (1 << 30), -1)]
    lines = [f"E {s} {r}" for s, r in cases] + [f"S {e}" for e in es] + [f"I {a} {b}" for a, b in idx] + [f"A {a}" for a, _ in args]
    lines += ["P 0 0 16", "P 4 0 16", "P 0 300 8", "P 0 255 8", "T"]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.check_output([exe], input="\n".join(lines).encode(), timeout=120, env=env).decode().strip().split("\n")
    assert len(out) == len(lines)
    it = iter(out)
    for s, r in cases:
        assert int(next(it)) == (512 * s + r * nc.L) // (2 * r * nc.L), (s, r)
    for e in es:
        assert next(it).split() == [str((e + 2 ** 20) >> 21), str((e + 2 ** 21) >> 22)]
    for a, b in idx:
        phi = (a * (b & nc.M32)) & nc.M32
        assert int(next(it)) == (((phi + (1 << 17)) & nc.M32) >> 18)
    for a, rc in args:
        assert int(next(it).split()[0]) == rc, a
    assert [int(next(it)) for _ in range(4)] == [64 << 20, 16 << 20, 256, 0]
    c, s = nc.lo_table()
    i = np.arange(1, c.size + 1)
    assert [int(v) for v in next(it).split()] == [int((c * i).sum()), int((s * i).sum())]


def test_header_and_binding_name_the_same_entries():
    src = open(os.path.join(ROOT, "include", "bds_mi355x.h")).read()
    assert re.search(r"BDS_NOTCH_DEV_API\s+int\s+bds_notch_dev\s*\(", src) and native.NOTCH_DEVICE_EXPORTS == ["bds_notch_dev"]
    for name in ("MAX_TONES", "MIN_LOG2", "MAX_LOG2", "PHASE_BITS", "LO_LOG2", "AMP_FRAC", "RUN_BYTES"):
        assert int(re.search(r"#define BDS_NOTCH_%s (\d+)" % name, src).group(1)) == getattr(native, "NOTCH_" + name), name
    assert (native.NOTCH_MAX_TONES, native.NOTCH_MIN_LOG2, native.NOTCH_MAX_LOG2, native.NOTCH_PHASE_BITS, native.NOTCH_LO_LOG2, native.NOTCH_AMP_FRAC) == (8, 8, 16, 14, 14, 8)
    for entry in ("bds_notch", "bds_notch_file", "bds_notch_lo"):
        assert re.search(r"BDS_API\s+int\s+%s\s*\(" % entry, src) and entry in native.EXPORTS and hasattr(native.lib(), entry), entry
    assert hasattr(native.lib(), "bds_notch_dev") and callable(getattr(native.Context, "notch", None))
    assert C.sizeof(native.NotchOpts) == 56 and C.sizeof(native.NotchOut) == 56
    for name in ("notch_tones", "notch_step", "notch_detect", "notch_refine", "NotchReport"):
        assert hasattr(bds_amd, name), name


def test_cw_tones_is_deterministic_and_conjugate():
    s = nc.settings_of("s8", samplingFreq=25e6, IF=6.5e6)
    tones = [(0.4e6, 60.0, 1.0), (-1.1e6, 7.5, -0.3)]
    a, b = synth.cw_tones(s, 5000, tones), synth.cw_tones(s, 5000, tones)
    assert a.dtype == np.float64 and np.array_equal(a, b)
    z, zc = synth.cw_tones(s, 5000, tones, iq_sign=1), synth.cw_tones(s, 5000, tones, iq_sign=-1)
    assert z.dtype == np.complex128 and np.array_equal(zc, np.conj(z)) and np.allclose(z.real, a, atol=1e-9)
    n = np.arange(5000)
    np.testing.assert_allclose(a, 60 * np.cos(2 * np.pi * 6.9e6 * n / 25e6 + 1.0) + 7.5 * np.cos(2 * np.pi * 5.4e6 * n / 25e6 - 0.3), atol=1e-6)
    np.testing.assert_allclose(synth.cw_tones(s, 100, tones, first_sample=4900), a[4900:], atol=1e-6)
    assert not synth.cw_tones(s, 5000, []).any() and synth.cw_tones(s, 5000, [], iq_sign=1).dtype == np.complex128
    assert synth.cw_tones(s, 0, tones).size == 0


def _welch(x, fs, cplx):
    """pwelch(x, 32768, 2048, 32768, fs) as probe_data computes it: (psd, freq)."""
    nfft, hop = 32768, 32768 - 2048
    w = 0.54 - 0.46 * np.cos(2 * np.pi * np.arange(nfft) / (nfft - 1))
    k = (x.size - 2048) // hop
    acc = np.zeros(nfft)
    for j in range(k):
        acc += np.abs(np.fft.fft(x[j * hop:j * hop + nfft] * w)) ** 2
    psd = acc / k / (fs * (w * w).sum())
    if not cplx:
        psd = psd[:nfft // 2 + 1].copy()
        psd[1:-1] *= 2
    return SimpleNamespace(psd=psd, freq=np.arange(psd.size) * fs / nfft)


def test_notch_detect_on_psds_computed_here():
    fs, n = 25e6, 2048 + 8 * 30720
    bin_hz = fs / 32768
    s = nc.settings_of("s8", samplingFreq=fs, IF=6.5e6)
    rng = np.random.default_rng(5)
    noise = rng.normal(0.0, 20.0, n)
    assert bds_amd.notch_detect(_welch(noise, fs, False), s) == []
    tones = [(6.9e6 + 317.0, 40.0), (2.2e6, 12.0), (11.05e6 + 111.0, 4.0)]
    t = np.arange(n) / fs
    x = noise + sum(a * np.cos(2 * np.pi * f * t + 0.4) for f, a in tones)
    got = bds_amd.notch_detect(_welch(x, fs, False), s)
    assert len(got) == 3
    for (f, _), g in zip(tones, got):  # strongest first
        assert abs(g - f) <= bin_hz, (f, g)
    assert bds_amd.notch_detect(_welch(x, fs, False), s, max_tones=2) == got[:2]
    sq = nc.settings_of("s8c", samplingFreq=fs, IF=0.0)
    zn = rng.normal(0.0, 20.0, n) + 1j * rng.normal(0.0, 20.0, n)
    assert bds_amd.notch_detect(_welch(zn, fs, True), sq) == []
    ztones = [(-3.3e6 - 50.0, 30.0), (1.7e6, 10.0), (-150.0, 5.0)]  # a negative frequency, a positive one, a line across DC
    z = zn + sum(a * np.exp(2j * np.pi * f * t) for f, a in ztones)
    got = bds_amd.notch_detect(_welch(z, fs, True), sq)
    assert len(got) == 3
    for (f, _), g in zip(ztones, got):
        assert abs(g - f) <= bin_hz, (f, g)


def test_notch_refine_recovers_a_planted_offset():
    """int8 real, sigma 6, amplitude A = 100, B = 1024, M = 256 blocks.  A block estimate is A/2 e^{j theta_b} (less the sinc of
    the offset) plus noise of variance (sigma^2 + 1/12) / (2 B) per component, so its phase carries
    sigma_phi = sqrt(2 (sigma^2 + 1/12) / B) / (A sinc) rad.  At this signal-to-noise ratio the angle of sum a[b] conj(a[b - 1]) is
    the mean phase step, which telescopes to (phi[M - 1] - phi[0]) / (M - 1): a deviation of sqrt(2) sigma_phi / (M - 1) rad per
    block, times fs / (2 pi B) in Hz.  The bound is six of those, plus the image's leak into each end estimate (1 / (pi D) rad at
    D = 2 f B / fs notch widths between the tone and its image, both ends), plus the step's own rounding fs / 2^33."""
    fs, B, M, A, sigma = 25e6, 1024, 256, 100.0, 6.0
    s = nc.settings_of("s8", samplingFreq=fs, IF=6.5e6)
    n = B * M
    f0 = 6.9e6
    for k, df in enumerate((100.0, 1000.0, 3000.0, -2000.0)):
        x = nc.noise("s8", n, seed=20 + k, sigma=sigma) + A * np.cos(2 * np.pi * (f0 + df) * np.arange(n) / fs + 0.9)
        rec = np.clip(np.rint(x), -127, 127).astype(np.int8)
        steps = [bds_amd.notch_step(f0, fs)]
        _, r = nc.model(rec, "s8", steps, 10, apply=False)
        rep = bds_amd.NotchReport(n_samples=n, n_blocks=M, n_saturated=0, sum_sq_in=r["sum_sq_in"], sum_sq_out=0,
                                  est=(r["est"][..., 0] + 1j * r["est"][..., 1]) / 256.0, steps=steps, tones=[f0], block=B)
        (got,) = bds_amd.notch_refine(rep, s)
        sinc = abs(np.sinc(df * B / fs))
        sigma_phi = math.sqrt(2 * (sigma ** 2 + 1 / 12) / B) / (A * sinc)
        image = 2.0 / (math.pi * 2 * f0 * B / fs)
        bound = (6 * math.sqrt(2) * sigma_phi + image) / (M - 1) * fs / (2 * math.pi * B) + fs / 2 ** 33
        print(f"offset {df}: refined to {got - f0:.3f} Hz, bound {bound:.3f} Hz")
        assert abs(got - (f0 + df)) <= bound, (df, got - f0, bound)


def test_scene_needs_the_excisor(scene):
    """peakMetric of PRN 9 on the float64 oracle: 1.91 clean, 1.00 jammed (a line of amplitude 60 at IF + 0.4 MHz over noise of
    sigma 20; the satellite at 44 dB-Hz), 1.91 notched by the model at B = 1024 (acqThreshold 1.5)"""
    s = scene.settings
    step = bds_amd.notch_step(scene.f_line, s.samplingFreq)
    notched, rep = nc.model(scene.jammed, "s8", [step], 10)
    assert rep["n_saturated"] == 0 and rep["sum_sq_in"] > 4 * rep["sum_sq_out"]
    clean = oacq.acquisition_b2a(scene.clean.astype(np.float64), s)
    jam = oacq.acquisition_b2a(scene.jammed.astype(np.float64), s)
    fix = oacq.acquisition_b2a(notched.astype(np.float64), s)
    print("peakMetric clean, jammed, notched:", clean.peakMetric[8], jam.peakMetric[8], fix.peakMetric[8])
    assert clean.carrFreq[8] != 0 and clean.peakMetric[8] > s.acqThreshold
    assert jam.carrFreq[8] == 0 and jam.peakMetric[8] < s.acqThreshold
    assert fix.carrFreq[8] != 0 and fix.peakMetric[8] >= s.acqThreshold + 0.25
    assert abs(fix.carrFreq[8] - (s.IF - 1230.0)) <= 50
