"""Tracking sessions without a GPU: the model of tests/track_session_cases.py against the oracle's whole-series C/N0 post-pass,
the header against its ctypes mirror, and the argument errors TrackSession raises before any native call."""
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import bds_amd
from bds_amd import native

from track_session_cases import CNO_INTERVAL, PIECES, n_cno_done, session_cno, whole_series_cno

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(total, tuple(pieces)) for total, lists in PIECES.items() for pieces in lists]
MORE = [(37, (3, 3, 3, 28)), (40, (9, 1, 10, 20)), (25, (25,)), (9, (4, 5))]  # ends inside an interval, on one, before the first


@pytest.mark.parametrize("total,pieces", CASES + MORE)
def test_intervals_per_call_sum_to_the_whole(total, pieces):
    assert sum(pieces) == total
    for M in sorted(set(CNO_INTERVAL.values()) | {2, 7}):
        done = n_cno_done(pieces, M)
        assert sum(done) == total // M
        assert all(0 <= d <= (k + M - 1) // M for d, k in zip(done, pieces))


@pytest.mark.parametrize("pilot_mode", [0, 1, 2])
@pytest.mark.parametrize("total,pieces", CASES + MORE)
def test_carried_prompts_give_the_whole_series_values(total, pieces, pilot_mode):
    """Exactly: the same M values reach the same function in the same order, whatever the pieces."""
    M = CNO_INTERVAL.get(total, 10)
    s = SimpleNamespace(CNoInterval=M, intTime=0.001)
    rng = np.random.default_rng(total * 7 + pilot_mode)
    # a tracked channel's prompts: a strong in-phase arm with data sign flips, a weak quadrature arm
    i_p = rng.choice([-1.0, 1.0], total) * 4000 + rng.normal(0, 300, total)
    q_p = rng.normal(0, 300, total)
    pil_i, pil_q = rng.normal(0, 300, total), 5000 + rng.normal(0, 300, total)
    want_cno, want_pld = whole_series_cno(i_p, q_p, pil_i, pil_q, s, pilot_mode)
    calls, left = session_cno(i_p, q_p, pil_i, pil_q, s, pilot_mode, pieces)
    assert [len(c) for c, _ in calls] == n_cno_done(pieces, M) and left == total % M
    np.testing.assert_array_equal(np.concatenate([c for c, _ in calls]), want_cno)
    np.testing.assert_array_equal(np.concatenate([p for _, p in calls]), want_pld)
    assert np.all(np.isfinite(want_cno[:, 0])) and len(want_cno) == total // M


# ---- header and mirror -----------------------------------------------------------------------------------------------------
SESSION_ENTRIES = {"bds_track_open": "track_open", "bds_track_open_mem": "track_open", "bds_track_open_feed": "track_open_feed",
                   "bds_track_feed": "track_feed", "bds_track_advance": "track_advance", "bds_track_session_info": "track_session_info",
                   "bds_track_close": "track_close"}


def test_every_session_entry_of_the_header_has_a_context_method():
    src = open(os.path.join(ROOT, "include", "bds_mi355x.h")).read()
    declared = set(re.findall(r"BDS_API\s+[\w\s\*]+?\b(bds_track_(?:open\w*|feed|advance|session_info|close))\s*\(", src))
    assert declared == set(SESSION_ENTRIES)
    lib = native.lib()
    for entry, method in SESSION_ENTRIES.items():
        assert entry in native.EXPORTS and hasattr(lib, entry), entry
        assert callable(getattr(native.Context, method)), method
    assert "typedef struct bds_track_session bds_track_session;" in src
    for name in ("TrackSession",):
        assert hasattr(bds_amd, name)
    for m in ("advance", "feed", "info", "close", "__enter__", "__exit__"):
        assert callable(getattr(bds_amd.TrackSession, m))


# ---- argument errors that need no library -----------------------------------------------------------------------------------
def _channels():
    return [SimpleNamespace(PRN=19, acquiredFreq=13.55e6, codePhase=101.0, codeFreq=10.23e6, status="T")]


@pytest.mark.parametrize("origin", [1, 31, 33, 48, -32, 64.5])
def test_origin_must_be_a_multiple_of_32(origin, monkeypatch):
    monkeypatch.setattr(sys.modules[bds_amd.TrackSession.__module__], "get_context", lambda *a: pytest.fail("no context is needed to refuse the origin"))
    with pytest.raises(ValueError, match="multiple of 32"):
        bds_amd.TrackSession(None, _channels(), bds_amd.init_settings_b2a(), origin=origin)
    with pytest.raises(ValueError, match="multiple of 32"):
        native.check_feed_origin(origin)
    assert [native.check_feed_origin(o) for o in (0, 32, 64, 3200)] == [0, 32, 64, 3200]


def test_source_and_origin_exclude_each_other(monkeypatch):
    monkeypatch.setattr(sys.modules[bds_amd.TrackSession.__module__], "get_context", lambda *a: pytest.fail("no context is needed"))
    with pytest.raises(ValueError, match="no source"):
        bds_amd.TrackSession(np.zeros(8, np.int8), _channels(), bds_amd.init_settings_b2a(), origin=64)
    with pytest.raises(ValueError, match="source is required"):
        bds_amd.TrackSession(None, _channels(), bds_amd.init_settings_b2a())


class _NoNative:
    """Stands where the Context would: any native call is a test failure."""

    def __getattr__(self, name):
        pytest.fail(f"Context.{name} reached: the argument error must be raised before any native call")


def _session(feed, file_type):
    """A TrackSession around a handle that was never opened: only the argument checks can run."""
    t = bds_amd.TrackSession.__new__(bds_amd.TrackSession)
    t._ctx = _NoNative()
    t._sess = {"handle": None, "n_ch": 1, "fileType": file_type, "keep": None, "feed": feed}
    return t


def test_feed_on_a_file_session_raises():
    t = _session(feed=False, file_type=1)
    with pytest.raises(ValueError, match="reads its record itself"):
        t.feed(np.zeros(64, np.int8))
    t._sess = None  # (nothing to close)


def test_odd_iq_byte_count_raises():
    sess = {"feed": True, "fileType": 2}
    with pytest.raises(ValueError, match="odd count"):
        native.check_feed_bytes(sess, np.zeros(1001, np.int8))
    assert native.check_feed_bytes(sess, np.zeros(1000, np.int8)).size == 1000
    assert native.check_feed_bytes({"feed": True, "fileType": 1}, np.zeros(1001, np.int8)).size == 1001
    assert native.check_feed_bytes({"feed": True, "fileType": 3}, np.arange(7, dtype=np.uint8)).dtype == np.int8
    with pytest.raises(ValueError, match="odd count"):
        native.Context.track_feed(_NoNative(), {"feed": True, "fileType": 2, "handle": None}, np.zeros(3, np.int8))


def test_closed_session_raises_with_a_message():
    t = _session(feed=True, file_type=1)
    t._sess = None
    for call in (lambda: t.advance(5), lambda: t.feed(np.zeros(4, np.int8)), t.info):
        with pytest.raises(native.BdsError, match="closed"):
            call()
    t.close()  # a second close does nothing
