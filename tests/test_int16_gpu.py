"""16-bit IF records (settings.dataType 'int16') on the GPU: tracking and acquisition of int16 samples, real and I/Q.

The arithmetic does not change with the sample width -- a sample becomes the same (double) value an int8 sample does -- so the
checks are exact wherever they can be (tests/int16_cases.py):
  embedding  an int16 record whose values fit int8 gives every output of the int8 run, bit for bit;
  scaling    256 x8 gives exactly 256 x the correlator sums and bit-equal scale-free outputs (tests/test_int16_cases.py shows the
             same on the float64 oracle);
and a record that uses all 16 bits is held against the oracle with the tolerances of tests/test_track_gpu.py and
tests/test_acq_gpu.py.  Shapes: the reduced-rate records of tests/helpers.py."""
import functools
import itertools

import numpy as np
import pytest
import torch

import bds_amd
from bds_amd import native, synth
from oracle import acquisition as oacq
from oracle import tracking as otrk

from helpers import as_complex, assert_closed_loop_parity, cfg1_b2a, cfg1_b2a_iq, resample_b1c, small_b1c, spc_of
from int16_cases import assert_scaled_results, case, embed, full, scale, settings16
from test_packed_gpu import assert_same_results, tuned
from test_track_gpu import CASES
from test_track_session_gpu import CNO_FIELDS, joined, joined_all

pytestmark = pytest.mark.gpu

GPU = "cuda:0"
SEG_CHUNK = {8: "2048", 16: "4096"}  # BDS_TRK_CHUNK of the two segment lengths of the run-based correlator
EMBED_EPOCHS = {"B2A": 20, "NB": 10, "WB": 10}  # one C/N0 interval each (CNoInterval 20 / 10)


def dev16(x16):
    """An int16 host array as an int16 tensor on the GPU."""
    return torch.from_numpy(np.array(x16, copy=True)).to(GPU)


def shifted(x, k, iq):
    """k samples (pairs) of junk in front of the record: with skipNumberOfBytes = k the channels start where they did, and a
    real int16 segment starts on the other half of a dword for odd k."""
    rng = np.random.default_rng(40 + k)
    junk = rng.integers(-100, 100, k * (2 if iq else 1)).astype(x.dtype)
    return np.concatenate([junk, x])


# ---- 1: embedding --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg", [8, 16])
@pytest.mark.parametrize("iq", [False, True], ids=["real", "iq"])
@pytest.mark.parametrize("mode", ["B2A", "NB", "WB"])
def test_embedded_int8_values_track_bit_equal(ctx, monkeypatch, mode, iq, seg):
    signal = "B2A" if mode == "B2A" else "B1C"
    s, s16, x8, chans = case(signal, mode, EMBED_EPOCHS[mode], iq)
    with tuned(ctx, monkeypatch, {"BDS_TRK_CHUNK": SEG_CHUNK[seg]}):
        for k in (0, 1, 2, 3):
            xk = shifted(x8, k, iq)
            want, _ = bds_amd.tracking(xk, chans, s.copy(skipNumberOfBytes=k), mode=mode)
            got, _ = bds_amd.tracking(embed(xk), chans, s16.copy(skipNumberOfBytes=k), mode=mode)
            assert [w.status for w in want] == ["T"] * 3 and np.all(want[0].absoluteSample[1:] > 0)
            assert_same_results(got, want)
    with tuned(ctx, monkeypatch, {"BDS_TRK_PERSAMPLE": "1"}):  # the per-sample kernel decodes the format at run time
        for k in (0, 1):
            xk = shifted(x8, k, iq)
            want, _ = bds_amd.tracking(xk, chans, s.copy(skipNumberOfBytes=k), mode=mode)
            got, _ = bds_amd.tracking(embed(xk), chans, s16.copy(skipNumberOfBytes=k), mode=mode)
            assert_same_results(got, want)


# ---- 2: scaling ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("signal,mode,n_epochs,iq", CASES)
def test_scaled_record_scales_the_correlators_only(ctx, signal, mode, n_epochs, iq):
    s, s16, x8, chans = case(signal, mode, n_epochs, iq)
    want, _ = bds_amd.tracking(x8, chans, s, mode=mode)
    got, _ = bds_amd.tracking(scale(x8), chans, s16, mode=mode)
    assert [w.status for w in want] == ["T"] * 3
    assert_scaled_results(got, want)


# ---- 3: all 16 bits against the oracle -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_full(signal, mode, n_epochs, iq):
    """The oracle on full(x8) (RawFile addresses the elements of the int16 array): (record, trackResults, per-epoch trace);
    computed once, shared and left unchanged."""
    s, s16, x8, chans = case(signal, mode, n_epochs, iq)
    x16 = full(x8)
    x16.setflags(write=False)
    trace = []
    ref, _ = otrk.tracking(otrk.RawFile(x16), chans, s16, mode=mode, trace=trace)
    return x16, ref, trace


@pytest.mark.parametrize("signal,mode,n_epochs,iq", CASES)
def test_open_loop_correlators_on_all_16_bits(ctx, signal, mode, n_epochs, iq):
    _, s16, _, chans = case(signal, mode, n_epochs, iq)
    x16, _, trace = oracle_full(signal, mode, n_epochs, iq)
    assert x16.min() == -32768 and x16.max() == 32767 and len(trace) == n_epochs * len(chans)
    for k in (1, n_epochs // 2, n_epochs):
        rows = [t for t in trace if t["k"] == k]
        prn = [chans[t["ch"]].PRN for t in rows]
        st = [[t["pos"], t["blk"], t["rem"], t["codeFreq"], t["remCarr"], t["carrFreq"]] for t in rows]
        got = ctx.track_correlate(s16, x16, prn, st)
        for g, t in zip(got, rows):
            p = np.hypot(t["sums"][2], t["sums"][3])
            np.testing.assert_allclose(g, t["sums"], rtol=0, atol=1e-6 * p)


@pytest.mark.parametrize("signal,mode,n_epochs,iq", CASES)
def test_closed_loop_on_all_16_bits(ctx, signal, mode, n_epochs, iq):
    _, s16, _, chans = case(signal, mode, n_epochs, iq)
    x16, ref, _ = oracle_full(signal, mode, n_epochs, iq)
    got, _ = bds_amd.tracking(x16, chans, s16, mode=mode)
    assert_closed_loop_parity(ref, got, mode)


# ---- 4: every way in -----------------------------------------------------------------------------------------------------
WAYS = [("B2A", "B2A", 60, False), ("B2A", "B2A", 40, True)]
FEED_PIECES = (1, 3, 4097, 65536)  # bytes the producer delivers per step: they split samples and pairs


@functools.lru_cache(maxsize=None)
def one_call(signal, mode, n_epochs, iq):
    """(int16 record, its one-window trackResults): computed once, shared and left unchanged."""
    _, s16, x8, chans = case(signal, mode, n_epochs, iq)
    x16 = full(x8)
    x16.setflags(write=False)
    ctx = bds_amd.get_context(0)
    want, _ = bds_amd.tracking(x16, chans, s16, mode=mode)
    assert ctx.track_stream_info()["pieces"] == 1 and [w.completed for w in want] == [n_epochs] * 3
    assert ctx.track_loaded_bytes() % (4 if iq else 2) == 0 and ctx.track_loaded_bytes() <= x16.nbytes
    return x16, want


def first_epochs(results, want, n, M):
    """A longer run cut to the n epochs of `want` (C/N0 arrays: the intervals that end inside them), status and count as want's."""
    out = []
    for r, w in zip(results, want):
        g = bds_amd.TrackResults()
        for f, wv in vars(w).items():
            rv = getattr(r, f)
            setattr(g, f, (rv[: n // M] if f in CNO_FIELDS else rv[:n]) if isinstance(wv, np.ndarray) else wv)
        assert r.completed >= n
        out.append(g)
    return out


@pytest.mark.parametrize("signal,mode,n_epochs,iq", WAYS, ids=["real", "iq"])
def test_file_stream_session_and_device_equal_the_one_call(ctx, tmp_path, signal, mode, n_epochs, iq):
    _, s16, _, chans = case(signal, mode, n_epochs, iq)
    x16, want = one_call(signal, mode, n_epochs, iq)
    unit = spc_of(s16) * (4 if iq else 2)  # bytes of one code period
    path = tmp_path / "record16.bin"
    x16.tofile(path)
    got, _ = bds_amd.tracking(str(path), chans, s16, mode=mode)
    assert_same_results(got, want)
    for source in (x16, str(path), dev16(x16)):  # streamed: a span buffer holds six periods
        got, _ = bds_amd.tracking(source, chans, s16, mode=mode, resident_limit=12 * unit)
        info = ctx.track_stream_info()
        assert info["pieces"] >= 3 and 0 < info["resident_max_bytes"] <= 12 * unit and info["repeated_batches"] == 0, info
        assert_same_results(got, want)
    got, _ = bds_amd.tracking(dev16(x16), chans, s16, mode=mode)  # bds_track_dev, one window
    assert_same_results(got, want)
    pieces = (7, 1, n_epochs - 21, 13)
    for source in (x16, str(path), dev16(x16)):  # bds_track_open_mem / _open / _open_dev, a moving span
        calls = []
        with bds_amd.TrackSession(source, chans, s16, resident_limit=12 * unit) as t:
            for n in pieces:
                calls.append(t.advance(n))
                assert t.last_k == n
        assert_same_results(joined(calls, want), want)


def feed_in_pieces(t, raw, sizes, unit, n_adv=7):
    """A producer delivers `raw` (uint8 or int16, host or device) in steps of `sizes` bytes (cycled); after every step the session
    is offered everything delivered and not yet taken, then advanced.  Every take is a whole number of samples."""
    item = raw.element_size() if hasattr(raw, "element_size") else raw.itemsize
    total = len(raw) * item
    calls, delivered, taken, takes = [], 0, 0, []
    for size in itertools.cycle(sizes):
        delivered = min(total, delivered + size)
        offered = raw[taken // item: delivered // item]
        took = t.feed(offered, last=delivered == total and (delivered - taken) % unit == 0)
        assert took % unit == 0 and 0 <= took <= len(offered) * item
        takes.append(took)
        taken += took
        r = t.advance(n_adv)
        if t.last_k:
            calls.append(r)
        assert took or t.last_k or (delivered - taken) < unit or delivered < total, "neither a byte taken nor an epoch run"
        if taken == total:
            break
    for _ in range(64):
        r = t.advance(n_adv)
        if not t.last_k:
            break
        calls.append(r)
    assert t.last_k == 0
    return calls, takes


@pytest.mark.parametrize("signal,mode,n_epochs,iq", WAYS, ids=["real", "iq"])
def test_feed_sessions_equal_the_one_call(ctx, signal, mode, n_epochs, iq):
    _, s16, _, chans = case(signal, mode, n_epochs, iq)
    x16, want = one_call(signal, mode, n_epochs, iq)
    unit = 4 if iq else 2
    M = int(s16.CNoInterval)
    raw = x16.view(np.uint8)
    with bds_amd.TrackSession(None, chans, s16, origin=0) as t:  # raw bytes in pieces that split samples and pairs
        calls, takes = feed_in_pieces(t, raw, FEED_PIECES, unit)
        assert t.info()["fed_end"] == x16.size // (2 if iq else 1)
    assert 0 in takes and sum(takes) == raw.size  # (a step of 1 byte offers no whole sample)
    assert_same_results(first_epochs(joined_all(calls), want, n_epochs, M), want)
    d16 = dev16(x16)
    with bds_amd.TrackSession(None, chans, s16, origin=0) as t:  # bds_track_feed_dev: int16 slices of a device tensor
        calls, _ = feed_in_pieces(t, d16, (65536, 4 * 4097), unit)
    assert_same_results(first_epochs(joined_all(calls), want, n_epochs, M), want)


def test_short_16_bit_file_returns_partial_results(ctx, tmp_path):
    """B2a/tracking.m:250-254 on a 16-bit record: the first channel keeps what it has, later channels never start, status '-'."""
    _, s16, x8, chans = case("B2A", "B2A", 40)
    x16 = full(x8)[: 25 * spc_of(s16)]
    ref, _ = otrk.tracking(otrk.RawFile(x16), chans, s16, mode="B2A")
    path = tmp_path / "short16.bin"
    x16.tofile(path)
    for source in (x16, str(path)):
        got, _ = bds_amd.tracking(source, chans, s16, mode="B2A")
        assert [g.status for g in got] == [r.status for r in ref] == ["-", "-", "-"]
        done = int(np.sum(np.isfinite(ref[0].carrFreq)))
        assert got[0].completed == done and 0 < done < 40
        np.testing.assert_array_equal(got[0].absoluteSample, ref[0].absoluteSample)
        np.testing.assert_allclose(got[0].I_P, ref[0].I_P, atol=1e-4 * np.abs(ref[0].I_P).max())
        for c in (1, 2):
            assert not np.any(got[c].I_P) and np.all(np.isinf(got[c].carrFreq))


# ---- 5: acquisition ------------------------------------------------------------------------------------------------------
ACQ = {"b2a": (cfg1_b2a, oacq.acquisition_b2a, False), "b2a_iq": (cfg1_b2a_iq, oacq.acquisition_b2a, True),
       "b1c": (small_b1c, oacq.acquisition_b1c, False)}


@functools.lru_cache(maxsize=None)
def acq_int8(name):
    """(settings, int8 block, acqResults of the int8 run): computed once, shared and left unchanged."""
    make, _, iq = ACQ[name]
    s, x8, _ = make()
    x8.setflags(write=False)
    return s, x8, bds_amd.acquisition(as_complex(x8) if iq else x8, s, verbose=False)


@pytest.mark.parametrize("kind", ["scale", "full"])
@pytest.mark.parametrize("name", list(ACQ))
def test_acquisition_of_a_16_bit_block(ctx, name, kind):
    _, oracle_fn, iq = ACQ[name]
    s, x8, got8 = acq_int8(name)
    s16 = settings16(s)
    x16 = scale(x8) if kind == "scale" else full(x8)
    block = as_complex(x16) if iq else x16  # (complex values: acquisition() interleaves them as int16 pairs)
    ref = oracle_fn(block.astype(np.complex128 if iq else np.float64), s16)
    got = bds_amd.acquisition(block, s16, verbose=False)
    tm = ctx.timing()
    assert tm["refine_path"] == 0 and tm["rows_kernel"] != 3 and tm["cols_kernel"] != 4, tm  # the L-point pair (3 / 4: an N-point pair), host refinement
    np.testing.assert_array_equal(got.codePhase, ref.codePhase)
    np.testing.assert_array_equal(got.carrFreq, ref.carrFreq)
    np.testing.assert_allclose(got.peakMetric, ref.peakMetric, rtol=1e-6, atol=0)
    assert np.count_nonzero(got.carrFreq) >= 1
    if kind == "scale":  # scale-free outputs (the two runs decide on different refinement paths)
        np.testing.assert_array_equal(got.codePhase, got8.codePhase)
        np.testing.assert_array_equal(got.carrFreq, got8.carrFreq)
        np.testing.assert_allclose(got.peakMetric, got8.peakMetric, rtol=1e-9, atol=0)
    on_dev = bds_amd.acquisition(dev16(x16), s16, verbose=False)  # bds_acq_load_dev: the same int16 values (pairs) in HBM
    for f in ("codePhase", "carrFreq", "peakMetric"):
        np.testing.assert_array_equal(getattr(on_dev, f), getattr(got, f), err_msg=f)


def test_resampling_branch_on_a_16_bit_block(ctx):
    """resamplingflag = 1: the filtfilt extension kernel reads int16 where it read int8."""
    s, x8, _ = resample_b1c()
    s16, x16 = settings16(s), full(x8)
    ref = oacq.acquisition_b1c(x16.astype(np.float64), s16)
    got = bds_amd.acquisition(x16, s16, verbose=False)
    np.testing.assert_array_equal(got.codePhase, ref.codePhase)
    np.testing.assert_array_equal(got.carrFreq, ref.carrFreq)
    np.testing.assert_allclose(got.peakMetric, ref.peakMetric, rtol=1e-6, atol=0)
    assert got.carrFreq[2] != 0 and got.carrFreq[11] != 0 and got.carrFreq[6] == 0


def test_acquire_track_on_a_16_bit_block_and_record(ctx, tmp_path):
    """bds_acquire_track16 equals acquisition, then pre_run, then tracking, done separately."""
    s = bds_amd.init_settings_b2a(samplingFreq=25e6, IF=6.5e6, acqSatelliteList=[5, 9, 19, 33], acqSearchBand=2500, fineNoncoh=5,
                                  msToProcess=40, numberOfChannels=3, CNoInterval=20, dataType="int16")
    sats = [synth.Sat(9, -1230.0, 12345.6, 2.0, 50.0), synth.Sat(19, 2210.0, 3001.2, 0.4, 47.0)]
    spc = spc_of(s)
    x16 = full(synth.make_if(s, sats, 60 * spc, seed=123))
    path = tmp_path / "record16.bin"
    x16.tofile(path)
    block = x16[: 8 * spc]
    acq, ch, trk = bds_amd.acquire_track(block, str(path), s)
    acq1 = bds_amd.acquisition(block, s, verbose=False)
    ch1 = bds_amd.pre_run(acq1, s)
    trk1, _ = bds_amd.tracking(str(path), ch1, s)
    for f in ("carrFreq", "codePhase", "peakMetric"):
        np.testing.assert_array_equal(getattr(acq, f), getattr(acq1, f), err_msg=f)
    key = lambda cc: [(c.PRN, c.codePhase, c.acquiredFreq, c.codeFreq, c.status) for c in cc]  # noqa: E731
    assert key(ch) == key(ch1) and sorted(c.PRN for c in ch) == [0, 9, 19]
    assert_same_results(trk, trk1)
    assert sorted(t.status for t in trk) == ["-", "T", "T"]
    _, _, trk2 = bds_amd.acquire_track(dev16(block), dev16(x16), s)  # block and record in HBM: three native calls, same results
    assert_same_results(trk2, trk1)


# ---- 6: refusals ---------------------------------------------------------------------------------------------------------
def test_refusals(ctx, monkeypatch, tmp_path):
    s, s16, x8, chans = case("B2A", "B2A", 20)
    x16 = embed(x8)
    loaded = ctx.track_loaded_bytes()

    def refused(call, code, *words):
        with pytest.raises(native.BdsError) as ei:
            call()
        assert ei.value.code == code, str(ei.value)
        for w in words:
            assert w in str(ei.value), str(ei.value)

    # dtype against setting, both directions, host and device arrays: raised before any copy
    for fid, st in ((x16, s), (x8, s16), (dev16(x16), s), (torch.from_numpy(np.array(x8)).to(GPU), s16)):
        refused(lambda: bds_amd.tracking(fid, chans, st), -1, "dataType")
        refused(lambda: bds_amd.TrackSession(fid, chans, st), -1, "dataType")
        refused(lambda: bds_amd.acquisition(fid, st, verbose=False), -1, "dataType")
    # fileType 3 has no 16-bit form: the array's dtype in Python, the settings in the library (a path goes by the setting alone)
    s3 = s16.copy(fileType=3)
    packed_path, odd_path, odd_iq_path = tmp_path / "packed.bin", tmp_path / "odd.bin", tmp_path / "odd_iq.bin"
    x8.view(np.uint8)[:100000].tofile(packed_path)
    refused(lambda: bds_amd.tracking(x8.view(np.uint8), chans, s3), -1, "dataType")
    refused(lambda: bds_amd.tracking(str(packed_path), chans, s3), -1, "fileType 3", "dataType")
    refused(lambda: ctx.acq_load(s16, x16, is_complex=2), -1, "is_complex = 2")
    # a record that is not a whole number of samples / pairs
    x16.view(np.uint8)[:-1].tofile(odd_path)
    x16.view(np.uint8)[:-2].tofile(odd_iq_path)
    assert (x16.nbytes - 2) % 4 == 2
    refused(lambda: bds_amd.tracking(str(odd_path), chans, s16), -1, "whole number", "int16 samples")
    refused(lambda: bds_amd.tracking(str(odd_iq_path), chans, s16.copy(fileType=2)), -1, "whole number", "pairs")
    with bds_amd.TrackSession(None, chans, s16, origin=0) as t:
        refused(lambda: t.feed(x16.view(np.uint8)[:4097], last=True), -1, "whole number")
        assert t.feed(x16.view(np.uint8)[:4097]) == 4096
    # the typed acquisition entries, and the multi-device one, keep their sample type
    cs8, cs16 = native.pack_settings(s), native.pack_settings(s16)
    lib, h = native.lib(), ctx._h
    p8, p16 = x8.ctypes.data_as(native.C.POINTER(native.C.c_int8)), x16.ctypes.data_as(native.C.POINTER(native.C.c_int16))
    refused(lambda: ctx._check(lib.bds_acq_load(h, native.C.byref(cs16), p8, x8.size, 0)), -3, "dataType", "bds_acq_load16")
    refused(lambda: ctx._check(lib.bds_acq_load16(h, native.C.byref(cs8), p16, x16.size, 0)), -1, "dataType")
    m = native.MultiContext([0])
    try:
        refused(lambda: m.acquire([(s16, x16, False)]), -3, "dataType")
    finally:
        m.close()
    refused(lambda: bds_amd.acquisition(x8, s.copy(dataType="float32"), verbose=False), -3, "dataType")
    # the 16-bit tracking kernels are built for the default numerics only
    for prec in ("0", "5"):
        with tuned(ctx, monkeypatch, {"BDS_TRK_PREC": prec}):
            refused(lambda: bds_amd.tracking(x16, chans, s16), -3, "BDS_TRK_PREC", "dataType")
            bds_amd.tracking(x8, chans, s)  # (int8 records run under every value)
    assert ctx.track_loaded_bytes() >= 0 and loaded >= 0
    got, _ = bds_amd.tracking(x16, chans, s16)  # the context works on
    assert [g.status for g in got] == ["T"] * 3
