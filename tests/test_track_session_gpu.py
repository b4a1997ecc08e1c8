"""Tracking sessions (bds_track_open* .. bds_track_close, bds_amd.TrackSession): a run advanced in pieces, or on samples fed by
the caller.  The contract under test: whatever the pieces, the concatenation of the arrays of successive advances equals the
arrays of ONE bds_track_mem call over the same epochs -- every comparison with the one-shot call below is assert_array_equal
over every field of trackResults, the C/N0 arrays with their smoothing across call boundaries included.

Shapes: B2a with the settings of BASELINE.json configs[0] (99.375 MS/s, 1-ms epochs), three satellites on four channels, 60
epochs, CNoInterval 10 (tests/track_session_cases.py); B1C at the reduced rate of tests/helpers.py, 12 epochs of 10 ms,
CNoInterval 4."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import bds_amd
from bds_amd import native
from bds_amd.tracking import TrackResults, field_set
from oracle import tracking as otrk

from helpers import assert_closed_loop_parity, spc_of
from packed_cases import packed_record
from test_packed_gpu import assert_same_results, tuned
from track_session_cases import (B2A_EPOCHS, CNO_INTERVAL, FEED_ADVANCE, FEED_CHUNK, PIECES, b1c_case, b2a_record, n_cno_done)

pytestmark = pytest.mark.gpu

CNO_FIELDS = ("DataCNo", "DataPLD", "PilotCNo", "PilotPLD", "B2a_CNo", "B1C_CNo")


def run_session(source, chans, s, pieces, mode=None, exact=True, **kw):
    """The per-call TrackResults lists of a session advanced by `pieces`, and its info at the end."""
    calls = []
    with bds_amd.TrackSession(source, chans, s, mode=mode, **kw) as t:
        for n in pieces:
            calls.append(t.advance(n))
            if exact:
                assert t.last_k == n
                assert [r.completed for r in calls[-1]] == [n if r.PRN else 0 for r in calls[-1]]
                assert [r.status for r in calls[-1]] == ["T" if r.PRN else "-" for r in calls[-1]]
        info = t.info()
    return calls, info


def joined(calls, want):
    """The calls' arrays end to end, as the trackResults list tracking() returns (an unused slot has no C/N0 interval in any call:
    its C/N0 arrays, empty here, stand as the one-shot call's zeros)."""
    out = []
    for c, w in enumerate(want):
        r = TrackResults()
        for f, wv in vars(w).items():
            if isinstance(wv, np.ndarray):
                v = np.concatenate([getattr(call[c], f) for call in calls])
                if w.PRN is None and f in CNO_FIELDS:
                    assert v.size == 0
                    v = wv
                setattr(r, f, v)
        r.PRN = calls[0][c].PRN
        r.completed = sum(call[c].completed for call in calls)
        r.status = "T" if all(call[c].status == "T" for call in calls) else "-"
        out.append(r)
    return out


def cut(results, n, M):
    """The first n epochs of a trackResults list (C/N0 arrays: the intervals that end inside them)."""
    out = []
    for w in results:
        r = TrackResults()
        for f, wv in vars(w).items():
            setattr(r, f, (wv[: n // M] if f in CNO_FIELDS else wv[:n]) if isinstance(wv, np.ndarray) else wv)
        out.append(r)
    return out


@functools.lru_cache(maxsize=None)
def b2a_want(iq=False):
    """One bds_track_mem call at 60 ms on the record of b2a_record(): computed once, shared and left unchanged."""
    s, x, chans = b2a_record(iq)
    want, _ = bds_amd.tracking(x, chans, s)
    assert [w.completed for w in want] == [B2A_EPOCHS] * 3 + [0]
    return want


# ---- 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pieces", PIECES[60], ids=lambda p: f"{len(p)}-pieces")
def test_b2a_pieces_equal_one_call(ctx, pieces):
    s, x, chans = b2a_record()
    want = b2a_want()
    calls, info = run_session(x, chans, s, pieces)
    assert_same_results(joined(calls, want), want)
    model = n_cno_done(pieces, CNO_INTERVAL[60])
    for c in range(3):
        assert [call[c].n_cno_done for call in calls] == model
        assert [len(call[c].DataCNo) for call in calls] == model
    assert [call[3].n_cno_done for call in calls] == [0] * len(pieces)
    assert list(info["epochs_done"]) == [60, 60, 60, 0]
    for c in range(3):  # the next epoch starts one block behind the last one tracked
        assert 0.9 * 99375 < info["next_sample"][c] - want[c].absoluteSample[-1] < 1.1 * 99375
    assert ctx.track_stream_info()["repeated_batches"] == 0


# ---- 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 4, 5])
@pytest.mark.parametrize("mode", ["NB", "WB"])
def test_b1c_pieces_equal_one_call(ctx, monkeypatch, mode, prec):
    s, x, chans = b1c_case(mode)
    with tuned(ctx, monkeypatch, {"BDS_TRK_PREC": str(prec)}):
        want, _ = bds_amd.tracking(x, chans, s, mode=mode)
        for pieces in PIECES[12]:
            calls, _ = run_session(x, chans, s, pieces, mode=mode)
            assert_same_results(joined(calls, want), want)
            assert [call[0].n_cno_done for call in calls] == n_cno_done(pieces, CNO_INTERVAL[12])


# ---- 3 ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def b2a_formats():
    """b2a_record as an I/Q record quantised to the packed alphabet: (fileType-2 settings, its int8 pairs, fileType-3 settings, the
    packed bytes, channels)."""
    s2, x_iq, chans = b2a_record(iq=True)
    packed, pairs = packed_record(x_iq)
    packed.setflags(write=False), pairs.setflags(write=False)
    return s2, pairs, s2.copy(fileType=3), packed, chans


@pytest.mark.parametrize("file_type", [2, 3])
def test_formats_and_a_moving_span(ctx, file_type):
    s2, pairs, s3, packed, chans = b2a_formats()
    s, x = (s2, pairs) if file_type == 2 else (s3, packed)
    want, _ = bds_amd.tracking(x, chans, s)
    assert [w.completed for w in want] == [B2A_EPOCHS] * 3 + [0]
    unit = spc_of(s) * 2 if file_type == 2 else spc_of(s) // 2  # bytes of one code period
    limit = 24 * unit  # a span buffer holds 12 periods: the advance of 39 epochs needs several, and so does the run
    pieces = PIECES[60][0]
    calls, seen = [], []
    with bds_amd.TrackSession(x, chans, s, resident_limit=limit) as t:
        for n in pieces:
            before = ctx.track_stream_info()["pieces"]
            calls.append(t.advance(n))
            assert t.last_k == n
            seen.append(ctx.track_stream_info()["pieces"] - before)
        info = ctx.track_stream_info()
        assert 0 < t.info()["resident_bytes"] <= limit // 2
    assert seen[-1] > 1 and sum(1 for v in seen if v) > 1, seen  # within the last advance, and across advances
    assert info["repeated_batches"] == 0 and 0 < info["resident_max_bytes"] <= limit, info
    assert ctx.track_resident_limit() == 0
    assert_same_results(joined(calls, want), want)


# ---- 4 ---------------------------------------------------------------------------------------------------------------
def test_file_source_equals_memory(ctx, tmp_path):
    s, x, chans = b2a_record()
    path = tmp_path / "record.bin"
    x.tofile(path)
    pieces = PIECES[60][0]
    from_file, _ = run_session(str(path), chans, s, pieces)
    from_mem, _ = run_session(x, chans, s, pieces)
    for a, b in zip(from_file, from_mem):
        assert_same_results(a, b)
    assert_same_results(joined(from_file, b2a_want()), b2a_want())


# ---- 5, 6 ------------------------------------------------------------------------------------------------------------
def minimum_limit(chans, s, origin=0):
    with pytest.raises(native.BdsError) as ei:
        bds_amd.TrackSession(None, chans, s, origin=origin, resident_limit=1)
    m = re.search(r"at least (\d+) bytes", str(ei.value))
    assert m, str(ei.value)
    return int(m.group(1))


def feed_all(t, data, chunk, n_adv):
    """Feed `data` in chunks of `chunk` bytes (the last with last=True), one advance(n_adv) after every feed call; then advance until
    nothing runs any more.  Returns (the calls that ran epochs, the number of feed calls that took fewer bytes than offered)."""
    calls, partial = [], 0
    for off in range(0, data.size, chunk):
        piece = data[off:off + chunk]
        is_last = off + chunk >= data.size
        while True:
            took = t.feed(piece, last=is_last)
            assert 0 <= took <= piece.size
            partial += took < piece.size
            r = t.advance(n_adv)
            if t.last_k:
                calls.append(r)
            assert took or t.last_k, "neither a byte taken nor an epoch run: the session is stuck"
            piece = piece[took:]
            if piece.size == 0:
                break
    for _ in range(8):
        r = t.advance(n_adv)
        if not t.last_k:
            break
        calls.append(r)
    assert t.last_k == 0
    return calls, partial


@functools.lru_cache(maxsize=None)
def oracle_blocks():
    """Whole blocks the float64 oracle reads for each channel of b2a_record() ALONE before its short read."""
    s, x, chans = b2a_record()
    out = []
    for ch in chans[:3]:
        r, _ = otrk.tracking(otrk.RawFile(x), [ch], s.copy(numberOfChannels=1, msToProcess=B2A_EPOCHS + 10))
        assert r[0].status == "-"  # it met the end of the record
        out.append(int(np.isfinite(r[0].remCodePhase).sum()))
    return out


def check_fed_run(calls, info, s, x, chans, origin=0):
    done = [sum(call[c].completed for call in calls) for c in range(4)]
    assert done == list(info["epochs_done"]) == oracle_blocks() + [0]  # every channel ends at its own short read
    assert all(d > B2A_EPOCHS for d in done[:3])
    e_min = min(done[:3])
    want, _ = bds_amd.tracking(x, chans, s.copy(msToProcess=e_min))
    assert [w.completed for w in want] == [e_min] * 3 + [0]
    got = cut(joined_all(calls), e_min, CNO_INTERVAL[60])
    for g, w in zip(got, want):
        g.completed, g.status = min(g.completed, e_min), w.status  # (the run went on past e_min: counted above)
        if w.PRN is None:
            for f in CNO_FIELDS:
                if hasattr(w, f):
                    setattr(g, f, getattr(w, f))
    assert_same_results(got, want)
    return e_min


def joined_all(calls):
    """The calls' arrays end to end, field set taken from the first call."""
    out = []
    for c in range(len(calls[0])):
        r = TrackResults()
        for f, v in vars(calls[0][c]).items():
            if isinstance(v, np.ndarray):
                setattr(r, f, np.concatenate([getattr(call[c], f) for call in calls]))
        r.PRN = calls[0][c].PRN
        r.completed = sum(call[c].completed for call in calls)
        r.status = "-"
        out.append(r)
    return out


def test_feed_at_the_minimum_limit(ctx):
    s, x, chans = b2a_record()
    # a first feed shorter than one block: nothing can run yet
    with bds_amd.TrackSession(None, chans, s, origin=0) as t:
        assert t.feed(x[:50_000]) == 50_000
        r = t.advance(FEED_ADVANCE)
        assert t.last_k == 0 and [q.completed for q in r] == [0] * 4 and list(t.info()["epochs_done"]) == [0] * 4
        assert t.info()["fed_end"] == 50_000
    minimum = minimum_limit(chans, s)
    # a span buffer holds the record from the origin to the latest start sample, plus one block at a code rate 2 % low, plus what
    # the blocks of a code rate 2 % high and 2 % low differ by
    latest = max(c.codePhase for c in chans[:3]) - 1
    assert 2 * (latest + 99375) < minimum < 2 * (latest + 1.1 * 99375)
    with bds_amd.TrackSession(None, chans, s, origin=0, resident_limit=minimum) as t:
        calls, partial = feed_all(t, x, FEED_CHUNK, FEED_ADVANCE)
        info = t.info()
        assert info["fed_end"] == x.size and info["resident_bytes"] <= minimum // 2
        with pytest.raises(native.BdsError, match="end of the record"):
            t.feed(x[:16])
    assert partial >= 1
    stream = ctx.track_stream_info()
    assert stream["resident_max_bytes"] <= minimum and stream["repeated_batches"] == 0, stream
    check_fed_run(calls, info, s, x, chans)


def test_feed_with_an_origin(ctx):
    """The same record fed from its sample 64 on: the channels start behind the origin, positions stay those of the record."""
    s, x, chans = b2a_record()
    assert min(c.codePhase for c in chans[:3]) - 1 > 64
    with bds_amd.TrackSession(None, chans, s, origin=64) as t:
        calls, _ = feed_all(t, x[64:], FEED_CHUNK, FEED_ADVANCE)
        info = t.info()
    assert info["fed_end"] == x.size
    check_fed_run(calls, info, s, x, chans)  # (absoluteSample among the fields: it counts from the record's sample 0)
    assert calls[0][0].absoluteSample[0] == chans[0].codePhase - 1
    with pytest.raises(native.BdsError, match="before origin_sample"):
        bds_amd.TrackSession(None, chans, s, origin=int(chans[2].codePhase) // 32 * 32 + 32)


# ---- 7 ---------------------------------------------------------------------------------------------------------------
def test_b2a_session_against_the_oracle(ctx):
    s, x, chans = b2a_record()
    ref, _ = otrk.tracking(otrk.RawFile(x), chans, s)
    calls, _ = run_session(x, chans, s, PIECES[60][0])
    got = joined(calls, b2a_want())
    assert_closed_loop_parity(ref[:3], got[:3], "B2A")


def test_wb_session_against_the_oracle(ctx):
    s, x, chans = b1c_case("WB")
    ref, _ = otrk.tracking(otrk.RawFile(x), chans, s, mode="WB")
    want, _ = bds_amd.tracking(x, chans, s, mode="WB")
    calls, _ = run_session(x, chans, s, PIECES[12][0], mode="WB")
    assert_closed_loop_parity(ref, joined(calls, want), "WB")


# ---- 8 ---------------------------------------------------------------------------------------------------------------
def test_acquire_between_two_advances(ctx):
    from helpers import cfg1_b2a

    s, x, chans = b2a_record()
    sa, xa, _ = cfg1_b2a()
    acq_alone = ctx.acquire(sa, xa)
    calls = []
    with bds_amd.TrackSession(x, chans, s) as t:
        calls.append(t.advance(23))
        acq_during = ctx.acquire(sa, xa)
        calls.append(t.advance(37))
    for a, b in zip(acq_during, acq_alone):
        np.testing.assert_array_equal(a, b)
    assert np.count_nonzero(acq_alone[3]) >= 1  # (it detected its satellite)
    assert_same_results(joined(calls, b2a_want()), b2a_want())


def test_one_shot_call_after_close_equals_a_fresh_context(ctx):
    s, x, chans = b2a_record()
    with bds_amd.TrackSession(x, chans, s, resident_limit=24 * spc_of(s)) as t:
        t.advance(17)
    after, _ = bds_amd.tracking(x, chans, s)
    assert ctx.track_stream_info()["pieces"] == 1
    fresh_ctx = native.Context(0)
    try:
        n, m, ep, cn, _ = field_set(s, "B2A")
        arr = fresh_ctx.track(s, x, chans, n, m, ep + cn)
    finally:
        fresh_ctx.close()
    for c, r in enumerate(after):
        for f in ep:
            np.testing.assert_array_equal(getattr(r, f), arr[f][c], err_msg=f)
        for f in cn:
            np.testing.assert_array_equal(getattr(r, "B2a_CNo" if f == "SigCNo" else f), arr[f][c], err_msg=f)
    assert_same_results(after, b2a_want())


def test_refused_calls_return_err_arg_with_a_message(ctx, tmp_path):
    s, x, chans = b2a_record()
    path = tmp_path / "record.bin"
    x[: 5 * 99375].tofile(path)
    lib = ctx._lib
    with bds_amd.TrackSession(x, chans, s) as t:
        first = t.advance(3)
        # a second open, the one-shot calls
        for call in (lambda: bds_amd.TrackSession(x, chans, s), lambda: bds_amd.TrackSession(None, chans, s, origin=0),
                     lambda: bds_amd.tracking(x, chans, s), lambda: bds_amd.tracking(str(path), chans, s)):
            with pytest.raises(native.BdsError, match="open tracking session") as ei:
                call()
            assert ei.value.code == -1
        # feed on a session that reads its record itself (the native check: TrackSession.feed raises before it)
        buf = np.zeros(64, dtype=np.int8)
        assert lib.bds_track_feed(t._sess["handle"], buf.ctypes.data_as(C.POINTER(C.c_int8)), buf.size, 0) == -1
        assert "reads its record itself" in lib.bds_last_error(ctx._h).decode()
        # C/N0 arrays too small for the intervals that can complete: refused before anything runs
        with pytest.raises(native.BdsError, match=r"n_cno = 1, but 3 C/N0 intervals") as ei:
            ctx.track_advance(t._sess, 30, 1, t._ep + t._cn)
        assert ei.value.code == -1 and list(t.info()["epochs_done"]) == [3, 3, 3, 0]
        second = t.advance(57)
        handle = t._sess["handle"]
        sess = dict(t._sess)
    assert_same_results(joined([first, second], b2a_want()), b2a_want())
    # any call after close: BDS_ERR_ARG, the handle is not read
    out, _ = ctx._track_out(4, 5, 1, ["absoluteSample", "I_P", "Q_P"])
    assert lib.bds_track_advance(handle, 5, C.byref(out), None) == -1
    assert lib.bds_track_feed(handle, None, 0, 0) == -1
    assert lib.bds_track_session_info(handle, None, None, None, None) == -1
    assert lib.bds_track_session_info(None, None, None, None, None) == -1
    lib.bds_track_close(handle)
    lib.bds_track_close(None)
    with pytest.raises(native.BdsError):
        ctx.track_advance(sess, 5, 1, ["absoluteSample", "I_P", "Q_P"])
    with pytest.raises(native.BdsError, match="closed"):
        t.advance(5)
    got, _ = bds_amd.tracking(x, chans, s)  # the context tracks again
    assert_same_results(got, b2a_want())
