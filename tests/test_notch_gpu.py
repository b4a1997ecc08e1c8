"""The tone excisor on the GPU against the NumPy model of tests/notch_cases.py, every comparison exact: bytes, guard bytes and
every integer of the report, the estimates included, in the four record formats, at the smallest shapes that reach every path
(partial last blocks, one to eight tones, the admitted limits of the steps, the workgroup's run of blocks, the largest block);
then the jammed B2a scene end to end -- detected, refined and notched in HBM, acquired and tracked from the same tensor."""
import ctypes as C

import numpy as np
import pytest
import torch

import bds_amd
from bds_amd import native, synth
from oracle import acquisition as oacq

import notch_cases as nc

pytestmark = pytest.mark.gpu

GPU = "cuda:0"
B = 256
N = 3 * B + 37
FMTS = list(nc.FORMATS)
KEYS = ("n_samples", "n_blocks", "n_saturated", "sum_sq_in", "sum_sq_out")


def dev(a, offset=0, guard=0xA5, tail=48):
    """(slice that holds `a` `offset` bytes into a guarded tensor, the whole uint8 tensor)"""
    raw = np.ascontiguousarray(a).view(np.uint8)
    big = torch.full((offset + raw.size + tail,), guard, dtype=torch.uint8, device=GPU)
    big[offset:offset + raw.size] = torch.from_numpy(raw.copy())
    t = big[offset:offset + raw.size]
    return (t.view(torch.int16) if a.dtype.itemsize == 2 else t.view(torch.int8)), big


def host(t, like):
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


def check(got, want):
    for k in KEYS:
        assert got[k] == want[k], (k, got[k], want[k])
    np.testing.assert_array_equal(got["est"], want["est"])


def run_dev(ctx, fmt, rec, steps, beta, offset=0, inplace=False, out_offset=None, **kw):
    """One bds_notch_dev call on a guarded device copy of rec: (output record on the host, report); the guards and, out of place,
    the input are checked here."""
    s = nc.settings_of(fmt)
    t, big = dev(rec, offset)
    oo = offset if out_offset is None else out_offset
    guarded = [(big, offset, 0xA5)]
    if inplace:
        out = t
    else:
        out, obig = dev(np.zeros_like(rec), oo, guard=0x3C)
        guarded.append((obig, oo, 0x3C))
    res, rep = ctx.notch(s, t, steps, beta, out=out, **kw)
    nb = rec.nbytes
    for b, o, g in guarded:
        assert bool((b[:o] == g).all()) and bool((b[o + nb:] == g).all()), "a byte outside the record was written"
    if not inplace:
        np.testing.assert_array_equal(host(t, rec), rec, err_msg="out of place changed its input")
    return host(out, rec), rep


@pytest.mark.parametrize("fmt", FMTS)
def test_sizes_tone_counts_and_the_admitted_limits(ctx, fmt):
    """steps_for puts the lowest and highest admitted step first and, for I/Q, a negative frequency and a tone exactly on the spacing limit"""
    for n in (1, B - 1, B, B + 1, N):
        for k in (1, 2, 8):
            steps = nc.steps_for(fmt, 8, k)
            rec = nc.with_tones(fmt, n, steps[:3], seed=n + k)
            want, wrep = nc.model(rec, fmt, steps, 8)
            got, rep = run_dev(ctx, fmt, rec, steps, 8)
            np.testing.assert_array_equal(got, want, err_msg=f"n={n} tones={k}")
            check(rep, wrep)
    if nc.FORMATS[fmt][3] == 1:  # the highest admitted step on its own
        steps = [(1 << 31) - 2 * nc.width(8)]
        rec = nc.with_tones(fmt, N, steps, seed=2)
        want, wrep = nc.model(rec, fmt, steps, 8)
        got, rep = run_dev(ctx, fmt, rec, steps, 8)
        np.testing.assert_array_equal(got, want)
        check(rep, wrep)


@pytest.mark.parametrize("fmt", ["s16", "s16c"])
def test_largest_block_with_every_component_at_the_minimum(ctx, fmt):
    """B = 65536, N = 2 B + 37, all -32768: a DC tone of the I/Q record sums to -2^45 per component, its estimate is -2^23"""
    beta, n = 16, 2 * 65536 + 37
    w = nc.width(beta)
    steps = [0, 4 * w + w // 3] if fmt == "s16c" else [2 * w, 9 * w + w // 3]
    rec = np.full(n * nc.FORMATS[fmt][3], -32768, dtype="<i2")
    want, wrep = nc.model(rec, fmt, steps, beta)
    if fmt == "s16c":
        assert wrep["est"][0, 0, 0] == -(1 << 23) and wrep["est"][0, 0, 1] == -(1 << 23)
    got, rep = run_dev(ctx, fmt, rec, steps, beta)
    np.testing.assert_array_equal(got, want)
    check(rep, wrep)


@pytest.mark.parametrize("fmt", ["s8", "s16c"])
def test_a_record_that_crosses_the_workgroups_run_of_blocks(ctx, fmt):
    beta = 10
    run = native.NOTCH_RUN_BYTES // ((1 << beta) * nc.sample_bytes(fmt))  # blocks per workgroup
    n = (run + 2) * (1 << beta) + 5
    steps = nc.steps_for(fmt, beta, 2)
    rec = nc.with_tones(fmt, n, steps, seed=6)
    want, wrep = nc.model(rec, fmt, steps, beta)
    got, rep = run_dev(ctx, fmt, rec, steps, beta, inplace=True)
    np.testing.assert_array_equal(got, want)
    check(rep, wrep)
    assert rep["n_blocks"] == run + 3


@pytest.mark.parametrize("fmt", FMTS)
def test_extreme_values_and_saturation(ctx, fmt):
    _, _, dt, c = nc.FORMATS[fmt]
    steps = nc.steps_for(fmt, 8, 2)
    for value in (np.iinfo(dt).min, np.iinfo(dt).max):
        rec = np.full(N * c, value, dtype=dt)
        want, wrep = nc.model(rec, fmt, steps, 8)
        got, rep = run_dev(ctx, fmt, rec, steps, 8)
        np.testing.assert_array_equal(got, want)
        check(rep, wrep)
    for r in (1, 2, 3):  # a last block of r samples at the minimum: of a real record it is estimated as all tone, and y = -x
        rec = np.concatenate([nc.noise(fmt, B, seed=8), np.full(r * c, np.iinfo(dt).min, dtype=dt)])
        want, wrep = nc.model(rec, fmt, steps[:1], 8)
        if c == 1 and r == 1:
            assert wrep["n_saturated"] == 1 and want[-1] == np.iinfo(dt).max
        got, rep = run_dev(ctx, fmt, rec, steps[:1], 8)
        np.testing.assert_array_equal(got, want)
        check(rep, wrep)


@pytest.mark.parametrize("fmt", FMTS)
def test_alignment_in_place_and_out_of_place(ctx, fmt):
    offsets = (1, 3, 16) if nc.FORMATS[fmt][2] == np.int8 else (2, 16)
    steps = nc.steps_for(fmt, 8, 2)
    rec = nc.with_tones(fmt, N, steps, seed=7)
    want, wrep = nc.model(rec, fmt, steps, 8)
    for off in (0,) + offsets:
        for kw in ({"inplace": True}, {}, {"out_offset": (off + offsets[0]) % 16}):
            got, rep = run_dev(ctx, fmt, rec, steps, 8, offset=off, **kw)
            np.testing.assert_array_equal(got, want, err_msg=f"offset {off} {kw}")
            check(rep, wrep)


@pytest.mark.parametrize("fmt", FMTS)
def test_estimate_only_leaves_the_output_alone(ctx, fmt):
    steps = nc.steps_for(fmt, 8, 3)
    rec = nc.with_tones(fmt, N, steps, seed=9)
    _, wrep = nc.model(rec, fmt, steps, 8, apply=False)
    _, full = nc.model(rec, fmt, steps, 8)
    np.testing.assert_array_equal(wrep["est"], full["est"])
    t, big = dev(rec, 16)
    res, rep = ctx.notch(nc.settings_of(fmt), t, steps, 8, apply=False)
    assert res is None and rep["sum_sq_out"] == 0 and rep["n_saturated"] == 0
    check(rep, wrep)
    # the library itself, handed an output buffer it must not touch
    fill = torch.full((rec.nbytes + 64,), 0x3C, dtype=torch.uint8, device=GPU)
    o, r = native.pack_notch(steps, 8, apply=False)
    est = native.notch_est(r, N, 8, len(steps))
    cs = native.pack_settings(nc.settings_of(fmt))
    assert ctx._lib.bds_notch_dev(ctx._h, C.byref(cs), C.c_void_p(t.data_ptr()), rec.nbytes, C.c_void_p(fill.data_ptr() + 32), C.byref(o), C.byref(r)) == 0
    assert bool((fill == 0x3C).all()) and bool((big[:16] == 0xA5).all()) and bool((big[16 + rec.nbytes:] == 0xA5).all())
    np.testing.assert_array_equal(host(t, rec), rec)
    np.testing.assert_array_equal(est, wrep["est"])
    assert (r.sum_sq_in, r.sum_sq_out, r.n_saturated) == (wrep["sum_sq_in"], 0, 0)


@pytest.mark.parametrize("fmt", FMTS)
def test_sources_and_pieces_agree_with_one_call(ctx, fmt, tmp_path):
    _, _, dt, c = nc.FORMATS[fmt]
    n = 5 * B + 37
    skip = 3  # (samples: an odd count, and for int8 real an odd byte offset)
    steps = nc.steps_for(fmt, 8, 3)
    rec = nc.with_tones(fmt, n, steps, seed=10)
    want, wrep = nc.model(rec, fmt, steps, 8)
    header = (np.arange(skip * c) + 77).astype(dt)
    src = tmp_path / "in.bin"
    np.concatenate([header, rec]).tofile(src)
    s, s_skip = nc.settings_of(fmt), nc.settings_of(fmt, skipNumberOfBytes=skip)
    for piece in (B, 2 * B, 2 * B + 17, 0):  # (2 B + 17 is rounded down to 2 B)
        dst = tmp_path / f"out_{piece}.bin"
        _, rep = ctx.notch(s_skip, str(src), steps, 8, out=str(dst), piece_samples=piece)
        back = np.fromfile(dst, dtype=dt)
        np.testing.assert_array_equal(back[:skip * c], header)
        np.testing.assert_array_equal(back[skip * c:], want)
        check(rep, wrep)
    _, rep = ctx.notch(s_skip, str(src), steps, 8, apply=False, piece_samples=B)
    np.testing.assert_array_equal(rep["est"], wrep["est"])
    assert rep["sum_sq_in"] == wrep["sum_sq_in"] and rep["sum_sq_out"] == 0
    got, rep = ctx.notch(s, rec, steps, 8)
    np.testing.assert_array_equal(got.view(dt), want)
    check(rep, wrep)
    inplace = rec.copy()
    res, r2 = bds_amd.notch_tones(inplace, s.copy(samplingFreq=2.0 ** 32), steps, block=B, out="inplace")  # (fs = 2^32: a tone's Hz are its step)
    assert res is inplace and r2.steps == steps and r2.block == B and r2.est.shape == (wrep["n_blocks"], 3)
    np.testing.assert_array_equal(inplace, want)
    np.testing.assert_array_equal(r2.est, (wrep["est"][..., 0] + 1j * wrep["est"][..., 1]) / 256.0)
    # a caller's own two pieces on the device, the second told where it starts
    cut = 2 * B
    out, est, tot = [], [], np.zeros(4, dtype=object)
    for a, b in ((0, cut), (cut, n)):
        t, _ = dev(rec[a * c:b * c])
        res, rep = ctx.notch(s, t, steps, 8, first_sample=a)
        assert res is t
        out.append(host(t, rec[a * c:b * c])), est.append(rep["est"])
        tot += [rep["n_blocks"], rep["n_saturated"], rep["sum_sq_in"], rep["sum_sq_out"]]
    np.testing.assert_array_equal(np.concatenate(out), want)
    np.testing.assert_array_equal(np.concatenate(est), wrep["est"])
    assert tuple(int(v) for v in tot) == (wrep["n_blocks"], wrep["n_saturated"], wrep["sum_sq_in"], wrep["sum_sq_out"])


def test_an_empty_window_changes_nothing(ctx, tmp_path):
    """No sample in the window: nothing is uploaded or launched, no block and no sum -- a host record of 0 bytes, and a file that
    is only its header, which goes through as it is."""
    s = nc.settings_of("s8")
    steps = nc.steps_for("s8", 8, 2)
    got, rep = ctx.notch(s, np.zeros(0, dtype=np.int8), steps, 8)
    assert got.size == 0 and rep["est"].shape == (0, 2, 2)
    assert (rep["n_samples"], rep["n_blocks"], rep["n_saturated"], rep["sum_sq_in"], rep["sum_sq_out"]) == (0, 0, 0, 0, 0)
    src, dst = tmp_path / "header.bin", tmp_path / "out.bin"
    np.array([100, -100, 100], dtype=np.int8).tofile(src)
    _, rep = ctx.notch(nc.settings_of("s8", skipNumberOfBytes=3), str(src), steps, 8, out=str(dst))
    assert dst.read_bytes() == src.read_bytes() and rep["est"].shape == (0, 2, 2)
    assert (rep["n_samples"], rep["n_blocks"], rep["n_saturated"], rep["sum_sq_in"], rep["sum_sq_out"]) == (0, 0, 0, 0, 0)


def test_the_same_call_twice_gives_the_same_bytes_and_sums(ctx):
    steps = nc.steps_for("s8c", 10, 8)
    rec = nc.with_tones("s8c", 70 * 1024 + 5, steps[:3], seed=11)
    a, ra = run_dev(ctx, "s8c", rec, steps, 10)
    b, rb = run_dev(ctx, "s8c", rec, steps, 10)
    np.testing.assert_array_equal(a, b)
    check(ra, rb)
    want, wrep = nc.model(rec, "s8c", steps, 10)
    np.testing.assert_array_equal(a, want)
    check(ra, wrep)


def test_refusals_on_the_device(ctx):
    s = nc.settings_of("s8")
    steps = nc.steps_for("s8", 8, 1)
    hostbuf = np.zeros(4096, dtype=np.int8)
    o, rep = native.pack_notch(steps, 8)
    cs = native.pack_settings(s)
    p = hostbuf.ctypes.data_as(C.c_void_p)
    assert ctx._lib.bds_notch_dev(ctx._h, C.byref(cs), p, hostbuf.size, p, C.byref(o), C.byref(rep)) == -1
    assert "not device memory" in ctx._lib.bds_last_error(ctx._h).decode()
    t = torch.zeros(4096, dtype=torch.int8, device=GPU)
    with pytest.raises(native.BdsError, match="overlap"):
        ctx.notch(s, t[:2048], steps, 8, out=t[1024:3072])
    with pytest.raises(native.BdsError, match="packed"):
        ctx.notch(s.copy(fileType=3), t.view(torch.uint8), steps, 8)
    with pytest.raises(native.BdsError, match="image"):
        ctx.notch(s, t, [5], 8)
    res, rep = ctx.notch(s, t, steps, 8)  # the context still works
    assert res is t and rep["sum_sq_in"] == 0 and rep["n_blocks"] == 16 and not rep["est"].any()


# ---- the jammed scene end to end ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    return nc.cw_scenario()


def test_scene_detected_refined_and_notched_in_hbm_is_acquired_like_the_model_notched_record(ctx, scene):
    s = scene.settings
    t = torch.from_numpy(scene.jammed.copy()).to(GPU)
    jam = bds_amd.acquisition(t, s, verbose=False)
    assert jam.carrFreq[8] == 0, "the jammed record should hide PRN 9"
    found = bds_amd.notch_detect(bds_amd.probe_data(t, s, n_time=0), s)
    assert len(found) == 1 and abs(found[0] - scene.f_line) <= s.samplingFreq / 32768
    none, coarse = bds_amd.notch_tones(t, s, found, block=scene.block, estimate_only=True)
    assert none is None
    np.testing.assert_array_equal(t.cpu().numpy(), scene.jammed)
    fine = bds_amd.notch_refine(coarse, s)
    # (8 ms are 195 full blocks; the bound of tests/test_notch_cases.py::test_notch_refine_recovers_a_planted_offset at sigma 20, A 60)
    sigma_phi = np.sqrt(2 * (400 + 1 / 12) / scene.block) / (scene.amp * abs(np.sinc((found[0] - scene.f_line) * scene.block / s.samplingFreq)))
    bound = (6 * np.sqrt(2) * sigma_phi + 2 / (np.pi * 2 * scene.f_line * scene.block / s.samplingFreq)) / (coarse.n_samples // scene.block - 1) \
        * s.samplingFreq / (2 * np.pi * scene.block) + s.samplingFreq / 2 ** 33
    assert abs(fine[0] - scene.f_line) <= bound, (fine[0] - scene.f_line, bound)
    res, rep = bds_amd.notch_tones(t, s, fine, block=scene.block, out="inplace")
    assert res is t
    want, wrep = nc.model(scene.jammed, "s8", rep.steps, 10)
    np.testing.assert_array_equal(t.cpu().numpy(), want)
    assert (rep.n_saturated, rep.sum_sq_in, rep.sum_sq_out) == (wrep["n_saturated"], wrep["sum_sq_in"], wrep["sum_sq_out"])
    assert rep.removed_db > 6.0
    got = bds_amd.acquisition(t, s, verbose=False)
    ref = oacq.acquisition_b2a(want.astype(np.float64), s)
    assert ref.carrFreq[8] != 0 and got.carrFreq[8] != 0
    np.testing.assert_array_equal(got.codePhase, ref.codePhase)
    np.testing.assert_array_equal(got.carrFreq, ref.carrFreq)
    np.testing.assert_allclose(got.peakMetric, ref.peakMetric, rtol=1e-6, atol=0)


def test_scene_tracking_of_the_notched_tensor_equals_tracking_of_the_model_notched_array(ctx, scene):
    """(a 34-ms record of its own, the satellite at 48 dB-Hz: the channel only has to lock, the comparison is bit for bit)"""
    s = scene.settings.copy(msToProcess=30, numberOfChannels=1)
    n = 34 * scene.spc
    x = synth.make_if_device(s, [synth.Sat(9, -1230.0, 12345.6, 2.0, 48.0)], n, seed=2)
    cw = synth.cw_tones(s, n, [(scene.f_line - s.IF, scene.amp, 1.0)])
    jammed = np.clip(np.rint(x.astype(np.float64) + cw), -127, 127).astype(np.int8)
    step = bds_amd.notch_step(scene.f_line, s.samplingFreq)
    want, wrep = nc.model(jammed, "s8", [step], 10)
    t, rep = bds_amd.notch_tones(torch.from_numpy(jammed).to(GPU), s, [scene.f_line], block=scene.block)
    np.testing.assert_array_equal(t.cpu().numpy(), want)
    assert rep.steps == [step] and rep.sum_sq_out == wrep["sum_sq_out"]
    acq = bds_amd.acquisition(t[:8 * scene.spc], s, verbose=False)
    assert acq.carrFreq[8] != 0
    chans = bds_amd.pre_run(acq, s)
    got, _ = bds_amd.tracking(t, chans, s)
    ref, _ = bds_amd.tracking(want, chans, s)
    assert got[0].completed >= 30 and got[0].PRN == 9
    for f, v in vars(ref[0]).items():
        if isinstance(v, np.ndarray):
            np.testing.assert_array_equal(getattr(got[0], f), v, err_msg=f)
