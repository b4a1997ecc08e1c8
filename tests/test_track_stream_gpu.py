"""Streamed tracking (bds_track_set_resident_limit): the IF record passes through a bounded resident span of HBM in pieces, the
next piece loading while the epochs of the current one run.  Both modes run the same kernels on the same samples with the same
partial-sum order and state, so every comparison with the one-window run below is assert_array_equal on EVERY field of
trackResults -- no tolerance.  Shapes: the reduced-rate ones of tests/test_track_gpu.py (B2a at 25 MS/s, spc = 25 000, three
channels whose start samples differ by up to 0.7 spc; B1C at 12.5 MS/s, spc = 125 000, 10-ms blocks)."""
import functools

import numpy as np
import pytest

import bds_amd
from bds_amd import native, synth
from oracle import tracking as otrk

from helpers import assert_closed_loop_parity, spc_of, track_case

pytestmark = pytest.mark.gpu


def assert_same_results(got, want):
    """Every field of every channel's trackResults, bit for bit (NaN and Inf of the template included)."""
    assert len(got) == len(want)
    for c, (g, w) in enumerate(zip(got, want)):
        assert sorted(vars(g)) == sorted(vars(w))
        for f, wv in vars(w).items():
            gv = getattr(g, f)
            if isinstance(wv, np.ndarray):
                np.testing.assert_array_equal(gv, wv, err_msg=f"channel {c} {f}")
            else:
                assert gv == wv, (c, f, gv, wv)


@functools.lru_cache(maxsize=None)
def case(signal, mode, n_epochs, iq):
    """(settings, record, channels, one-window trackResults): computed once, shared and left unchanged."""
    s, x, chans = track_case(signal, mode, n_epochs, iq=iq)
    x.setflags(write=False)
    ctx = bds_amd.get_context(0)
    assert ctx.track_resident_limit() == 0
    want, _ = bds_amd.tracking(x, chans, s, mode=mode)
    assert ctx.track_stream_info()["pieces"] == 1
    return s, x, chans, want


def unit(s):
    """Bytes of one code period of the record."""
    return spc_of(s) * (2 if int(s.fileType) == 2 else 1)


# ---- 1 ---------------------------------------------------------------------------------------------------------------
# limits in code periods of bytes -> fewest pieces: piece boundaries fall before, inside and at the end of some channel's block;
# the last limit is no multiple of 16 bytes
B2A_LIMITS = [(12.0, 0, 5), (7.5, 0, 8), (5.0, 0, 12), (7.5, 7, 8)]


@pytest.mark.parametrize("iq", [False, True])
@pytest.mark.parametrize("periods,odd,min_pieces", B2A_LIMITS)
def test_b2a_streamed_equals_one_window(ctx, tmp_path, iq, periods, odd, min_pieces):
    s, x, chans, want = case("B2A", "B2A", 60, iq)
    limit = int(periods * unit(s)) + odd
    path = tmp_path / "record.bin"
    x.tofile(path)
    for source in (x, str(path)):
        got, _ = bds_amd.tracking(source, chans, s, mode="B2A", resident_limit=limit)
        info = ctx.track_stream_info()
        assert info["pieces"] >= min_pieces, info
        assert 0 < info["resident_max_bytes"] <= limit, info
        assert info["repeated_batches"] == 0, info
        assert_same_results(got, want)
    assert ctx.track_resident_limit() == 0  # the limit of a call does not stay on the context


# ---- 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,n_epochs,iq", [("WB", 12, False), ("NB", 8, True)])
def test_b1c_streamed_equals_one_window(ctx, mode, n_epochs, iq):
    """10-ms blocks: a block is a large share of the span (4 code periods resident, two per span buffer)."""
    s, x, chans, want = case("B1C", mode, n_epochs, iq)
    limit = 4 * unit(s)
    got, _ = bds_amd.tracking(x, chans, s, mode=mode, resident_limit=limit)
    info = ctx.track_stream_info()
    assert info["pieces"] >= n_epochs // 2 and info["resident_max_bytes"] <= limit, info
    assert_same_results(got, want)


# ---- 3 ---------------------------------------------------------------------------------------------------------------
def test_streamed_wb_against_the_oracle(ctx):
    s, x, chans, _ = case("B1C", "WB", 12, False)
    ref, _ = otrk.tracking(otrk.RawFile(x), chans, s, mode="WB")
    got, _ = bds_amd.tracking(x, chans, s, mode="WB", resident_limit=4 * unit(s))
    assert ctx.track_stream_info()["pieces"] > 1
    assert_closed_loop_parity(ref, got, "WB")


# ---- 4 ---------------------------------------------------------------------------------------------------------------
def test_short_file_in_a_later_piece(ctx, tmp_path):
    """B2a/tracking.m:250-254 with the end of the file several pieces in: the first channel keeps what it has, later channels
    are never started, exactly as on the one-window path (the record of test_short_file_returns_partial_results)."""
    s, x, chans = track_case("B2A", "B2A", 40)
    x = x[: 25 * 25000]
    want, _ = bds_amd.tracking(x, chans, s, mode="B2A")
    assert [w.status for w in want] == ["-", "-", "-"] and 0 < want[0].completed < 40
    path = tmp_path / "short.bin"
    x.tofile(path)
    for source in (x, str(path)):
        got, _ = bds_amd.tracking(source, chans, s, mode="B2A", resident_limit=8 * unit(s))
        assert ctx.track_stream_info()["pieces"] >= 5
        assert_same_results(got, want)
        for c in (1, 2):
            assert got[c].completed == 0 and not np.any(got[c].I_P) and np.all(np.isinf(got[c].carrFreq))


# ---- 5 ---------------------------------------------------------------------------------------------------------------
def _long_record(tmp_path):
    """The record of test_only_the_window_of_a_long_record_is_loaded: junk, the signal at skipNumberOfBytes, 60 periods of junk."""
    s, x, chans = track_case("B2A", "B2A", 20)
    spc = 25000
    rng = np.random.default_rng(9)
    junk = lambda n: np.clip(np.rint(rng.normal(0, 20, n)), -127, 127).astype(np.int8)  # noqa: E731
    skip = 7 * spc
    long_rec = np.concatenate([junk(skip), x, junk(60 * spc)])
    path = tmp_path / "long_record.bin"
    long_rec.tofile(path)
    return s.copy(skipNumberOfBytes=skip), long_rec, str(path), chans


def test_long_record_loads_about_the_window(ctx, tmp_path):
    s, long_rec, path, chans = _long_record(tmp_path)
    want, _ = bds_amd.tracking(long_rec, chans, s, mode="B2A")
    window = ctx.track_loaded_bytes()
    limit = 6 * unit(s)
    for source in (long_rec, path):
        got, _ = bds_amd.tracking(source, chans, s, mode="B2A", resident_limit=limit)
        assert ctx.track_stream_info()["pieces"] >= 5
        assert ctx.track_loaded_bytes() <= window + limit // 2  # one piece: at most a span buffer, half the limit
        assert_same_results(got, want)


# ---- 6 ---------------------------------------------------------------------------------------------------------------
def test_limit_at_or_above_the_window_is_one_window(ctx):
    s, x, chans, want = case("B2A", "B2A", 60, False)
    bds_amd.tracking(x, chans, s, mode="B2A")
    window = ctx.track_loaded_bytes()
    for limit in (window, window + 1, 10 * window):
        got, _ = bds_amd.tracking(x, chans, s, mode="B2A", resident_limit=limit)
        info = ctx.track_stream_info()
        assert info["pieces"] == 1 and info["resident_max_bytes"] == window and ctx.track_loaded_bytes() == window, info
        assert_same_results(got, want)
    bds_amd.tracking(x, chans, s, mode="B2A", resident_limit=window - 1)
    assert ctx.track_stream_info()["pieces"] > 1


# ---- 7 ---------------------------------------------------------------------------------------------------------------
def test_limit_below_the_minimum(ctx):
    import re

    s, x, chans, want = case("B2A", "B2A", 60, False)
    with pytest.raises(native.BdsError) as ei:
        bds_amd.tracking(x, chans, s, mode="B2A", resident_limit=2 * unit(s))  # a span buffer of one period: no room for the 0.7-period spread
    m = re.search(r"at least (\d+) bytes", str(ei.value))
    assert m, str(ei.value)
    minimum = int(m.group(1))
    # spread of the start samples (17 111) + one block at a code rate 2 % low + what a span start can fall behind, twice
    assert 2 * (17111 + 25000) < minimum < 2 * (17111 + 1.1 * 25000)
    with pytest.raises(native.BdsError):
        bds_amd.tracking(x, chans, s, mode="B2A", resident_limit=minimum - 1)
    got, _ = bds_amd.tracking(x, chans, s, mode="B2A", resident_limit=minimum)
    info = ctx.track_stream_info()
    assert info["pieces"] >= 30 and info["resident_max_bytes"] <= minimum, info
    assert_same_results(got, want)


# ---- 8 ---------------------------------------------------------------------------------------------------------------
def test_batch_repeated_after_the_window_guard(ctx, monkeypatch, tmp_path):
    """BDS_TRK_STREAM_MARGIN=0 plans every epoch that starts inside the span, so a block runs past it, the update kernel's
    window guard fires and the host repeats the batch from the state it started with: same bits, and no whole-file load."""
    if not native.has_test_hooks():
        pytest.skip("needs the test-hooks build")
    s, long_rec, path, chans = _long_record(tmp_path)
    want, _ = bds_amd.tracking(long_rec, chans, s, mode="B2A")
    window = ctx.track_loaded_bytes()
    limit = 6 * unit(s)
    monkeypatch.setenv("BDS_TRK_STREAM_MARGIN", "0")
    ctx.reload_tuning()
    try:
        for source in (long_rec, path):
            got, _ = bds_amd.tracking(source, chans, s, mode="B2A", resident_limit=limit)
            info = ctx.track_stream_info()
            assert info["repeated_batches"] > 0 and info["pieces"] >= 5 and info["resident_max_bytes"] <= limit, info
            assert ctx.track_loaded_bytes() <= window + limit // 2
            assert_same_results(got, want)
    finally:
        monkeypatch.delenv("BDS_TRK_STREAM_MARGIN")
        ctx.reload_tuning()


def test_window_that_cannot_be_allocated_is_streamed(ctx, monkeypatch):
    """The automatic rule: when the one-window allocation fails (test hook) the call streams instead of returning
    BDS_ERR_NOMEM -- with no limit set."""
    if not native.has_test_hooks():
        pytest.skip("needs the test-hooks build")
    s, x, chans, want = case("B2A", "B2A", 60, True)
    monkeypatch.setenv("BDS_TRK_WINDOW_NOMEM", "1")
    ctx.reload_tuning()
    try:
        got, _ = bds_amd.tracking(x, chans, s, mode="B2A")
        assert ctx.track_stream_info()["resident_max_bytes"] > 0
        assert_same_results(got, want)
    finally:
        monkeypatch.delenv("BDS_TRK_WINDOW_NOMEM")
        ctx.reload_tuning()
    got, _ = bds_amd.tracking(x, chans, s, mode="B2A")
    assert ctx.track_stream_info()["pieces"] == 1
    assert_same_results(got, want)


# ---- 9 ---------------------------------------------------------------------------------------------------------------
def test_acquire_track_with_a_limit(ctx, tmp_path):
    """bds_acquire_track streams like bds_track (two satellites on three channels: one channel stays idle)."""
    s = bds_amd.init_settings_b2a(samplingFreq=25e6, IF=6.5e6, acqSatelliteList=[5, 9, 19, 33], acqSearchBand=2500,
                                  fineNoncoh=5, msToProcess=40, numberOfChannels=3, CNoInterval=20)
    sats = [synth.Sat(9, -1230.0, 12345.6, 2.0, 50.0), synth.Sat(19, 2210.0, 3001.2, 0.4, 47.0)]
    spc = spc_of(s)
    x = synth.make_if(s, sats, 60 * spc, seed=123)
    path = tmp_path / "record.bin"
    x.tofile(path)
    block = x[: 8 * spc]
    acq, ch, trk = bds_amd.acquire_track(block, str(path), s)
    assert ctx.track_stream_info()["pieces"] == 1
    acq1, ch1, trk1 = bds_amd.acquire_track(block, str(path), s, resident_limit=8 * spc)
    assert ctx.track_stream_info()["pieces"] >= 5
    for f in ("carrFreq", "codePhase", "peakMetric"):
        np.testing.assert_array_equal(getattr(acq1, f), getattr(acq, f))
    assert [(c.PRN, c.codePhase, c.acquiredFreq, c.codeFreq, c.status) for c in ch1] == \
           [(c.PRN, c.codePhase, c.acquiredFreq, c.codeFreq, c.status) for c in ch]
    assert sorted(c.PRN for c in ch) == [0, 9, 19]
    assert_same_results(trk1, trk)


# ---- 10 --------------------------------------------------------------------------------------------------------------
def test_default_context_runs_one_window(ctx, tmp_path):
    s, x, chans, want = case("B2A", "B2A", 60, False)
    assert ctx.track_resident_limit() == 0
    path = tmp_path / "record.bin"
    x.tofile(path)
    for source in (x, str(path)):
        got, _ = bds_amd.tracking(source, chans, s, mode="B2A")
        info = ctx.track_stream_info()
        assert info["pieces"] == 1 and info["repeated_batches"] == 0, info
        assert_same_results(got, want)
