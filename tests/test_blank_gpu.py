"""The pulse blanker on the GPU against the NumPy model of tests/blank_cases.py, every comparison exact: bytes, guard bytes, and
every number of the report, in the four record formats, on records of 3 T + 37 samples (T = the kernels' tile) with the cases
placed at the tile seams; then the jammed B2a scene end to end -- blanked in HBM, acquired and tracked from the same tensor."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import bds_amd
from bds_amd import native, synth
from oracle import acquisition as oacq

import blank_cases as bc

pytestmark = pytest.mark.gpu

GPU = "cuda:0"
T = bc.T
N = 3 * T + 37
FMTS = list(bc.FORMATS)
BIG = native.BLANK_MAX_WINDOW
WINDOWS = [(0, 0), (1, 1), (25, 25), (T - 1, T - 1), (T, T), (T + 1, T + 1), (3 * T, 3 * T), (BIG, BIG), (0, T + 1), (3 * T, 0), (1, 25), (T - 1, 1)]
HITS = {"start": [0], "end": [N - 1], "seam": [T - 1, T], "mid": [T + 77, 2 * T + 5], "low": [10], "high": [N - 12]}


def dev(a, offset=0, guard=0xA5, tail=32):
    """(slice that holds `a` `offset` bytes into a guarded tensor, the whole uint8 tensor)"""
    raw = np.ascontiguousarray(a).view(np.uint8)
    big = torch.full((offset + raw.size + tail,), guard, dtype=torch.uint8, device=GPU)
    big[offset:offset + raw.size] = torch.from_numpy(raw.copy())
    t = big[offset:offset + raw.size]
    return (t.view(torch.int16) if a.dtype.itemsize == 2 else t.view(torch.int8)), big


def host(t, like):
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


def check(got, want):
    for k in ("n_samples", "n_flagged", "n_blanked", "n_runs"):
        assert got[k] == want[k], (k, got[k], want[k])
    if want["duty"] is not None:
        np.testing.assert_array_equal(got["duty"], want["duty"])


def run_dev(ctx, fmt, rec, tsq, pre, post, offset=0, inplace=False, out_offset=None, **kw):
    """One bds_blank_dev call on a guarded device copy of rec: (output record on the host, report); the guards and, out of place,
    the input are checked here."""
    s = bc.settings_of(fmt)
    t, big = dev(rec, offset)
    oo = offset if out_offset is None else out_offset
    guarded = [(big, offset, 0xA5)]
    if inplace:
        out = t
    else:
        out, obig = dev(np.zeros_like(rec), oo, guard=0x3C)
        guarded.append((obig, oo, 0x3C))
    res, rep = ctx.blank(s, t, tsq, pre, post, out=out, **kw)
    nb = rec.nbytes
    for b, o, g in guarded:
        assert bool((b[:o] == g).all()) and bool((b[o + nb:] == g).all()), "a byte outside the record was written"
    if not inplace:
        np.testing.assert_array_equal(host(t, rec), rec, err_msg="out of place changed its input")
    return host(out, rec), rep


@pytest.mark.parametrize("fmt", FMTS)
def test_windows_and_flag_placement(ctx, fmt):
    for name, hits in HITS.items():
        rec = bc.with_hits(fmt, N, hits, seed=3)
        for pre, post in WINDOWS:
            want, wrep = bc.model(rec, fmt, 2500, pre, post, duty_samples=1000)
            got, rep = run_dev(ctx, fmt, rec, 2500, pre, post, duty_samples=1000)
            np.testing.assert_array_equal(got, want, err_msg=f"{name} pre={pre} post={post}")
            check(rep, wrep)


@pytest.mark.parametrize("fmt", FMTS)
def test_none_all_and_one_run_against_two(ctx, fmt):
    rec = bc.quiet(fmt, N, seed=4)
    got, rep = run_dev(ctx, fmt, rec, 2500, 25, 25)
    np.testing.assert_array_equal(got, rec)
    assert (rep["n_flagged"], rep["n_blanked"], rep["n_runs"]) == (0, 0, 0)
    full = np.full_like(rec, 100)
    want, wrep = bc.model(full, fmt, 2500, 0, 0, duty_samples=N)
    got, rep = run_dev(ctx, fmt, full, 2500, 0, 0, duty_samples=N)
    np.testing.assert_array_equal(got, want)
    check(rep, wrep)
    assert rep["n_blanked"] == N and rep["n_runs"] == 1 and not got.any()
    for first in (100, T - 4, 2 * T - 1):  # inside a tile, across a seam, the last sample of a tile
        for gap, runs in ((3 + 5 + 1, 1), (3 + 5 + 2, 2)):
            r2 = bc.with_hits(fmt, N, [first, first + gap], seed=5)
            want, wrep = bc.model(r2, fmt, 2500, 3, 5)
            got, rep = run_dev(ctx, fmt, r2, 2500, 3, 5)
            np.testing.assert_array_equal(got, want)
            check(rep, wrep)
            assert rep["n_runs"] == runs


@pytest.mark.parametrize("fmt", FMTS)
def test_extreme_values_and_thresholds(ctx, fmt):
    _, _, dt, c = bc.FORMATS[fmt]
    lowest = np.iinfo(dt).min
    rec = bc.quiet(fmt, N, seed=6)
    for h in (5, T - 1, T, N - 1):
        rec[h * c:(h + 1) * c] = lowest  # -128 / -32768 in every component
    p = c * lowest * lowest  # 2^31 for int16 pairs
    for tsq, flagged in ((p - 1, 4), (p, 0)):
        want, wrep = bc.model(rec, fmt, tsq, 2, 2)
        got, rep = run_dev(ctx, fmt, rec, tsq, 2, 2)
        np.testing.assert_array_equal(got, want)
        check(rep, wrep)
        assert rep["n_flagged"] == flagged
    want, wrep = bc.model(rec, fmt, 0, 0, 0, duty_samples=1000)  # threshold_sq = 0: every sample that is not 0
    got, rep = run_dev(ctx, fmt, rec, 0, 0, 0, duty_samples=1000)
    np.testing.assert_array_equal(got, want)
    check(rep, wrep)
    assert not got.any() and 0 < rep["n_flagged"] < N


@pytest.mark.parametrize("fmt", FMTS)
def test_alignment_in_place_and_out_of_place(ctx, fmt):
    offsets = (1, 3, 15) if bc.FORMATS[fmt][2] == np.int8 else (2, 14)
    rec = bc.with_hits(fmt, N, [0, 9, T - 1, T, 2 * T + 3, N - 1], seed=7)
    for pre, post in ((25, 25), (T + 1, 0), (0, 0)):
        want, wrep = bc.model(rec, fmt, 2500, pre, post, duty_samples=1000)
        for off in (0,) + offsets:
            for kw in ({"inplace": True}, {}, {"out_offset": (off + offsets[0]) % 16}):
                got, rep = run_dev(ctx, fmt, rec, 2500, pre, post, offset=off, duty_samples=1000, **kw)
                np.testing.assert_array_equal(got, want, err_msg=f"offset {off} {kw}")
                check(rep, wrep)


@pytest.mark.parametrize("fmt", FMTS)
def test_lead_tail_pieces_equal_the_whole(ctx, fmt):
    c = bc.FORMATS[fmt][3]
    rec = bc.with_hits(fmt, N, [0, 40, 4999, 5000, 5026, 9990, T - 1, T, T + 5030, 2 * T + 3, N - 1], seed=8)
    s = bc.settings_of(fmt)
    pre, post, piece = 30, 25, 5000
    want, wrep = bc.model(rec, fmt, 2500, pre, post)
    out, tot = [], np.zeros(3, dtype=np.int64)
    for a in range(0, N, piece):
        b = min(N, a + piece)
        l0, l1 = max(0, a - post - 1), min(N, b + pre)
        t, _ = dev(rec[l0 * c:l1 * c])
        res, rep = ctx.blank(s, t, 2500, pre, post, out=None, lead=a - l0, tail=l1 - b)
        assert rep["n_samples"] == b - a
        out.append(host(res, rec[l0 * c:l1 * c])[(a - l0) * c:(b - l0) * c])
        tot += [rep["n_flagged"], rep["n_blanked"], rep["n_runs"]]
    np.testing.assert_array_equal(np.concatenate(out), want)
    assert tuple(tot) == (wrep["n_flagged"], wrep["n_blanked"], wrep["n_runs"])


@pytest.mark.parametrize("fmt", FMTS)
def test_sources_file_host_and_tensor_agree(ctx, fmt, tmp_path):
    _, _, dt, c = bc.FORMATS[fmt]
    skip = 3  # (samples: an odd count, and for int8 real an odd byte offset)
    s = bc.settings_of(fmt, skipNumberOfBytes=skip)
    rec = bc.with_hits(fmt, N, [0, 4990, 5020, T - 1, T, 2 * T + 3, N - 1], seed=9)
    header = (np.arange(skip * c) + 77).astype(dt)
    src, pre, post = tmp_path / "in.bin", 25, 25
    np.concatenate([header, rec]).tofile(src)
    for ds in (1, 1000, N):
        want, wrep = bc.model(rec, fmt, 2500, pre, post, duty_samples=ds)
        got_h, rep_h = ctx.blank(bc.settings_of(fmt), rec, 2500, pre, post, duty_samples=ds)
        np.testing.assert_array_equal(got_h.view(dt), want)
        check(rep_h, wrep)
        got_t, rep_t = run_dev(ctx, fmt, rec, 2500, pre, post, duty_samples=ds)
        np.testing.assert_array_equal(got_t, want)
        check(rep_t, wrep)
        for piece in (0, 5000, 5010):  # (5010: samples 4990 and 5020 make one run across the seam)
            dst = tmp_path / f"out_{ds}_{piece}.bin"
            _, rep_f = ctx.blank(s, str(src), 2500, pre, post, out=str(dst), duty_samples=ds, piece_samples=piece)
            back = np.fromfile(dst, dtype=dt)
            np.testing.assert_array_equal(back[:skip * c], header)
            np.testing.assert_array_equal(back[skip * c:], want)
            check(rep_f, wrep)
    inplace = rec.copy()
    res, rep = bds_amd.blank_pulses(inplace, bc.settings_of(fmt), threshold=50.0, pre=pre, post=post, out="inplace")
    assert res is inplace and rep.threshold_sq == 2500
    np.testing.assert_array_equal(inplace, bc.model(rec, fmt, 2500, pre, post)[0])


def test_an_empty_window_changes_nothing(ctx, tmp_path):
    """No sample in the window: nothing is uploaded or launched, every byte goes through and every count is 0 -- a host array that
    is all context, and a file that is only its header."""
    s = bc.settings_of("s8")
    rec = np.full(64, 100, dtype=np.int8)  # every sample above the threshold, none owned
    got, rep = ctx.blank(s, rec, 2500, 3, 3, lead=40, tail=24, duty_samples=8)
    np.testing.assert_array_equal(got, rec)
    assert (rep["n_samples"], rep["n_flagged"], rep["n_blanked"], rep["n_runs"]) == (0, 0, 0, 0) and rep["duty"].size == 0  # (n_duty bins)
    src, dst = tmp_path / "header.bin", tmp_path / "out.bin"
    np.array([100, -100, 100], dtype=np.int8).tofile(src)
    _, rep = ctx.blank(bc.settings_of("s8", skipNumberOfBytes=3), str(src), 2500, 3, 3, out=str(dst), duty_samples=8)
    assert dst.read_bytes() == src.read_bytes()
    assert (rep["n_samples"], rep["n_flagged"], rep["n_blanked"], rep["n_runs"]) == (0, 0, 0, 0) and rep["duty"].size == 0


def test_windows_across_the_groups_of_the_tile_scan(ctx):
    """The scan over the tile summaries has two levels, groups of 1024 tiles: a record of three groups with hits at the group seams
    and windows that reach across them (the smallest size at which the second level does anything)."""
    g = 1024 * T
    n = 2 * g + 5
    hits = [g - 10, g + 2, 2 * g - 1, 2 * g + 3, 77]
    for fmt, (pre, post) in (("s8", (BIG, 3)), ("s8", (T + 1, BIG))):
        rec = bc.with_hits(fmt, n, hits, seed=12)
        want, wrep = bc.model(rec, fmt, 2500, pre, post, duty_samples=g - 1)
        t = torch.from_numpy(rec).to(GPU)
        res, rep = ctx.blank(bc.settings_of(fmt), t, 2500, pre, post, duty_samples=g - 1)
        assert res is t
        np.testing.assert_array_equal(t.cpu().numpy(), want)
        check(rep, wrep)


def test_refusals_on_the_device(ctx):
    s = bc.settings_of("s8")
    hostbuf = np.zeros(4096, dtype=np.int8)
    o, rep, _ = native.pack_blank(2500, 1, 1)
    cs = native.pack_settings(s)
    p = hostbuf.ctypes.data_as(C.c_void_p)
    assert ctx._lib.bds_blank_dev(ctx._h, C.byref(cs), p, hostbuf.size, p, C.byref(o), C.byref(rep)) == -1
    assert "not device memory" in ctx._lib.bds_last_error(ctx._h).decode()
    t = torch.zeros(4096, dtype=torch.int8, device=GPU)
    with pytest.raises(native.BdsError, match="overlap"):
        ctx.blank(s, t[:2048], 2500, 1, 1, out=t[1024:3072])
    with pytest.raises(native.BdsError, match="packed"):
        ctx.blank(s.copy(fileType=3), t.view(torch.uint8), 2500, 1, 1)
    res, rep = ctx.blank(s, t, 2500, 1, 1)  # the context still works
    assert res is t and rep["n_blanked"] == 0


# ---- the jammed scene end to end ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    sc = bc.dme_scenario()
    sc.blanked, sc.report = bc.model(sc.jammed, "s8", sc.threshold ** 2, sc.pre, sc.post)
    return sc


def test_scene_blanked_in_hbm_is_acquired_like_the_model_blanked_record(ctx, scene):
    s = scene.settings
    t = torch.from_numpy(scene.jammed.copy()).to(GPU)
    jam = bds_amd.acquisition(t, s, verbose=False)
    assert jam.carrFreq[8] == 0, "the jammed record should hide PRN 9"
    res, rep = bds_amd.blank_pulses(t, s, threshold=scene.threshold, pre=scene.pre, post=scene.post, out="inplace")
    assert res is t
    np.testing.assert_array_equal(t.cpu().numpy(), scene.blanked)
    assert (rep.n_flagged, rep.n_blanked, rep.n_runs) == (scene.report["n_flagged"], scene.report["n_blanked"], scene.report["n_runs"])
    got = bds_amd.acquisition(t, s, verbose=False)
    ref = oacq.acquisition_b2a(scene.blanked.astype(np.float64), s)
    assert ref.carrFreq[8] != 0 and got.carrFreq[8] != 0
    np.testing.assert_array_equal(got.codePhase, ref.codePhase)
    np.testing.assert_array_equal(got.carrFreq, ref.carrFreq)
    np.testing.assert_allclose(got.peakMetric, ref.peakMetric, rtol=1e-6, atol=0)


def test_scene_tracking_of_the_blanked_tensor_equals_tracking_of_the_model_blanked_array(ctx, scene):
    """(a 34-ms record of its own, the satellite at 48 dB-Hz: the channel only has to lock, the comparison is bit for bit)"""
    s = scene.settings.copy(msToProcess=30, numberOfChannels=1)
    n = 34 * scene.spc
    x = synth.make_if_device(s, [synth.Sat(9, -1230.0, 12345.6, 2.0, 48.0)], n, seed=2)
    p = synth.dme_pulses(s, n, pairs_per_s=20000, peak=400, f_offset=1e6, seed=7)
    jammed = np.clip(np.rint(x.astype(np.float64) + p), -127, 127).astype(np.int8)
    want, wrep = bc.model(jammed, "s8", scene.threshold ** 2, scene.pre, scene.post)
    t, rep = bds_amd.blank_pulses(torch.from_numpy(jammed).to(GPU), s, threshold=scene.threshold, pre=scene.pre, post=scene.post)
    np.testing.assert_array_equal(t.cpu().numpy(), want)
    assert abs(rep.fraction - 0.25) < 0.02
    acq = bds_amd.acquisition(t[:8 * scene.spc], s, verbose=False)
    assert acq.carrFreq[8] != 0
    chans = bds_amd.pre_run(acq, s)
    got, _ = bds_amd.tracking(t, chans, s)
    ref, _ = bds_amd.tracking(want, chans, s)
    assert got[0].completed >= 30 and got[0].PRN == 9
    for f, v in vars(ref[0]).items():
        if isinstance(v, np.ndarray):
            np.testing.assert_array_equal(getattr(got[0], f), v, err_msg=f)
