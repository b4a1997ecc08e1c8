"""Records in device memory (bds_synth_dev, bds_acq_load_dev, bds_track_dev, bds_track_open_dev, bds_track_feed_dev and their
Python routing): each entry against its host-memory counterpart on the same bytes.  The contract is bit-equality, so every
comparison below is assert_array_equal (assert_same_results over every field of trackResults); the one tolerance is the float64
oracle's in the chain test, which is helpers.assert_closed_loop_parity as tests/test_track_session_gpu.py uses it.

Device arrays are torch tensors on GPU 0, mostly slices that start an odd number of bytes into a larger tensor (the library accepts
any byte alignment), and in places a bare __cuda_array_interface__ object over such a slice."""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

import bds_amd
from bds_amd import native, synth
from bds_amd.tracking import TrackResults
from oracle import tracking as otrk

from helpers import assert_closed_loop_parity, cfg1_b2a, cfg1_b2a_iq, spc_of, track_case
from packed_cases import packed_record
from track_session_cases import CNO_INTERVAL, FEED_ADVANCE, FEED_CHUNK, PIECES, b1c_case, b2a_record

pytestmark = pytest.mark.gpu

GPU = "cuda:0"
CNO_FIELDS = ("DataCNo", "DataPLD", "PilotCNo", "PilotPLD", "B2a_CNo", "B1C_CNo")


# ---- device arrays -------------------------------------------------------------------------------------------------------
def dev(x, offset=0):
    """The bytes of a host array as a device tensor of the same dtype (int8 / uint8) that starts `offset` bytes into a larger one."""
    a = np.array(x, copy=True).reshape(-1)
    assert a.dtype in (np.int8, np.uint8)
    big = torch.empty(offset + a.size + 16, dtype=torch.uint8, device=GPU)
    big[offset:offset + a.size] = torch.from_numpy(a.view(np.uint8))
    t = big[offset:offset + a.size]
    return t.view(torch.int8) if a.dtype == np.int8 else t


class RawSpan:
    """A bare __cuda_array_interface__ object: n elements of `typestr` at a pointer (of a device tensor kept alive in `owner`)."""

    def __init__(self, ptr, n, typestr="|i1", owner=None):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": typestr, "data": (int(ptr), False), "version": 3, "strides": None}


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


# ---- 1. generator --------------------------------------------------------------------------------------------------------
FIRST = 12345
SEED = 3550
SYNTH_KW = {0: {"clean": True}, 1: {}, 2: {"iq_sign": 1}, 3: {"iq_sign": -1, "packed": True}}
ITEM = {0: 8, 1: 1, 2: 1, 3: 1}
TYPESTR = {0: "<f8", 1: "|i1", 2: "|i1", 3: "|u1"}


def _b1c_record(fmt):
    """The B1C record of tests/test_synth_gpu.py: 30.69 MS/s, two satellites, 2 x 306 900 + 77 samples (format 3: the even count next to it)."""
    s = bds_amd.init_settings_b1c(samplingFreq=30.69e6, IF=7.5e6)
    n = 2 * 306900 + 77
    return s, [synth.Sat(3, 1250.0, 100.0, 0.7, 47.0), synth.Sat(27, -4321.5, 20000.25, 2.9, 44.0)], n - 1 if fmt == 3 else n


@functools.lru_cache(maxsize=None)
def host_record(fmt):
    """bds_synth's host result: made once per format, shared and left unchanged."""
    s, sats, n = _b1c_record(fmt)
    x = synth.make_if_device(s, sats, n, seed=SEED, first_sample=FIRST - (fmt == 3), **SYNTH_KW[fmt])
    x.setflags(write=False)
    return x


def _elements(fmt, n):
    return {0: n, 1: n, 2: 2 * n, 3: n // 2}[fmt]


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_generator_out_torch_equals_the_host_record(ctx, fmt):
    s, sats, n = _b1c_record(fmt)
    want = host_record(fmt)
    t = synth.make_if_device(s, sats, n, seed=SEED, first_sample=FIRST - (fmt == 3), out="torch", **SYNTH_KW[fmt])
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.device.index == 0
    assert t.dtype == {0: torch.float64, 1: torch.int8, 2: torch.int8, 3: torch.uint8}[fmt] and tuple(t.shape) == want.shape
    np.testing.assert_array_equal(t.cpu().numpy(), want)
    tm = ctx.timing()
    assert tm["forward_ms"] > 0 and tm["search_ms"] >= 0 and tm["total_ms"] == tm["forward_ms"] + tm["search_ms"]
    # whole 16-byte units into a fresh allocation: written in place, no copy made
    k = synth.make_if_device(s, sats, 4096, seed=SEED, first_sample=FIRST - (fmt == 3), out="torch", **SYNTH_KW[fmt])
    assert k.data_ptr() % 16 == 0 and ctx.timing()["search_ms"] == 0 and ctx.timing()["forward_ms"] > 0
    np.testing.assert_array_equal(k.cpu().numpy(), want[:k.numel()])
    with pytest.raises(ValueError, match="out must be"):
        synth.make_if_device(s, sats, 64, out="cupy", **SYNTH_KW[fmt])


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_generator_into_a_misaligned_slice_leaves_its_surroundings_alone(ctx, fmt):
    """The record written 1, 3 and 5 bytes into a larger tensor of sentinels (and once at offset 0, where whole 16-byte units are
    written in place and only the last partial one is copied): the record is the host's, every byte around it is untouched."""
    s, sats, n = _b1c_record(fmt)
    want = host_record(fmt).view(np.uint8)
    tail = 37
    for off in (1, 3, 5, 0):
        big = torch.full((off + want.size + tail,), 0xA5, dtype=torch.uint8, device=GPU)
        span = RawSpan(big.data_ptr() + off, _elements(fmt, n), TYPESTR[fmt], owner=big)
        assert want.size == _elements(fmt, n) * ITEM[fmt]
        ctx.synth_dev(s, sats, FIRST - (fmt == 3), n, fmt, span, seed=SEED, **{k: v for k, v in SYNTH_KW[fmt].items() if k == "iq_sign"})
        got = big.cpu().numpy()
        np.testing.assert_array_equal(got[off:off + want.size], want, err_msg=f"offset {off}")
        assert np.all(got[:off] == 0xA5) and np.all(got[off + want.size:] == 0xA5), off


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_generator_in_three_pieces_equals_one_call(ctx, fmt):
    s, sats, n = _b1c_record(fmt)
    want = host_record(fmt)
    first = FIRST - (fmt == 3)
    cuts = [0, 4097, 70001, n] if fmt != 3 else [0, 4098, 70002, n]
    out = torch.zeros(want.size, dtype=getattr(torch, want.dtype.name), device=GPU)
    for a, b in zip(cuts[:-1], cuts[1:]):
        piece = out[_elements(fmt, a):_elements(fmt, b)]  # (formats 1 and 3: an odd byte offset into the tensor)
        ctx.synth_dev(s, sats, first + a, b - a, fmt, piece, seed=SEED, **{k: v for k, v in SYNTH_KW[fmt].items() if k == "iq_sign"})
    np.testing.assert_array_equal(out.cpu().numpy(), want)


# ---- 2. acquisition ------------------------------------------------------------------------------------------------------
def _acq(ctx, s, x, prns, is_complex=0):
    ctx.acq_load(s, x, is_complex)
    ctx.acq_prepare(s)
    res = ctx.acq_run(s, prn_list=prns)
    tm = ctx.timing()
    grid, arg = ctx.acq_grid(len(prns), int(tm["n_bins"]))
    pk, dn, fb = ctx.acq_peaks(63)
    return res, tm, grid.copy(), arg.copy(), pk, dn, fb


def _assert_same_acq(a, b):
    for u, v in zip(a[0], b[0]):
        np.testing.assert_array_equal(u, v)  # carrFreq, codePhase, peakMetric, detected
    for i in (2, 3, 4, 5, 6):                 # the sieve's grid and arguments, f64 peaks, second peaks, winning bins
        np.testing.assert_array_equal(a[i], b[i])
    for k in ("rows_kernel", "cols_kernel", "fft_len", "n_circ", "n_bins", "refine_path", "half_storage", "plan_l1", "plan_l2"):
        assert a[1][k] == b[1][k], k


def _host_and_device(ctx, s, x, prns, is_complex=0, offset=0):
    assert not native.is_device_array(x)
    host = _acq(ctx, s, x, prns, is_complex)
    d = dev(x, offset)
    assert native.is_device_array(d) and d.data_ptr() % 2 == offset % 2
    got = _acq(ctx, s, d, prns, is_complex)
    _assert_same_acq(got, host)
    return host


@pytest.fixture(scope="module")
def cfg1():
    return cfg1_b2a()


@pytest.mark.parametrize("offset", [0, 1])
def test_acq_load_b2a_cfg1(ctx, cfg1, offset):
    s, x, _ = cfg1
    assert x.size == 993750 and list(s.acqSatelliteList) == [19]
    host = _host_and_device(ctx, s, x, [19], offset=offset)
    assert host[1]["n_bins"] == 3 and host[0][0][18] != 0
    # the f64 coherent sums of caller-chosen cells read the loaded block: the same after either load
    cells = (19, 36771, [s.IF - 400.0, s.IF, s.IF + 400.0], 0)
    z_dev = ctx.acq_coherent_sums(s, *cells)
    _acq(ctx, s, x, [19])
    np.testing.assert_array_equal(z_dev, ctx.acq_coherent_sums(s, *cells))
    assert np.abs(z_dev).max() > 0


def test_acq_load_b1c_on_the_n_point_pair(ctx):
    """The block of tests/test_pfa32_gpu.py: B1C at the 53 MS/s defaults, a +-400 Hz band (17 bins), PRNs 19, 20, 35."""
    s0 = bds_amd.init_settings_b1c()
    spc = spc_of(s0)
    sats = [synth.Sat(19, -308.0, 0.613 * spc, 0.7, 47.0), synth.Sat(35, 210.0, 0.2 * spc, 2.0, 46.0), synth.Sat(46, 13770.0, 0.41 * spc, 1.1, 47.0)]
    x = synth.make_if(s0, sats, 4 * spc, seed=53)
    s = s0.copy(acqSatelliteList=list(range(1, 64)), acqSearchBand=400.0)
    host = _host_and_device(ctx, s, x, [19, 20, 35], offset=3)
    assert (host[1]["rows_kernel"], host[1]["cols_kernel"], host[1]["fft_len"], host[1]["n_bins"]) == (3, 4, 1060000, 17)
    assert host[0][0][19 - 1] != 0 and host[0][0][35 - 1] != 0 and host[0][0][20 - 1] == 0


def test_acq_load_iq_pairs_and_packed_bytes(ctx):
    s, x, _ = cfg1_b2a_iq()
    assert x.size == 2 * 993750
    prns = [19, 20, 21]
    host = _host_and_device(ctx, s, x, prns, is_complex=1, offset=1)
    assert host[0][0][18] != 0 and host[0][0][19] != 0 and host[0][0][20] == 0
    packed, _ = packed_record(x)
    host3 = _host_and_device(ctx, s.copy(fileType=3), packed, prns, is_complex=2, offset=5)
    assert host3[0][0][18] != 0
    # the count checks are the host's: an odd number of int8 values is no I/Q record, n_samples beyond the array is refused
    with pytest.raises(ValueError, match="odd count"):
        ctx.acq_load(s, dev(x[:-1]), 1)
    with pytest.raises(ValueError, match="holds"):
        ctx.acq_load(s, dev(x), 1, n_samples=x.size)
    with pytest.raises(ValueError, match="uint8"):
        bds_amd.acquisition(dev(x), s.copy(fileType=3), verbose=False)


def test_acq_load_with_the_resampling_branch(ctx, cfg1):
    s, x, _ = cfg1
    s = s.copy(resamplingflag=1)
    assert native.resample_plan(s) is not None
    host = _host_and_device(ctx, s, x, [19], offset=1)
    plain = _acq(ctx, s.copy(resamplingflag=0), x, [19])
    assert host[1]["fft_len"] != plain[1]["fft_len"] and host[0][0][18] != 0  # (the search ran on the resampled block)


# ---- 3. tracking ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def track_record(name):
    """(settings, record bytes, channels, mode, epochs): b2a_record() as it is (fileType 1), b1c_case("NB") as an I/Q record
    (fileType 2) and b1c_case("WB") as a packed record (fileType 3) -- the same satellites, channels and cuts as b1c_case's."""
    if name == "b2a-ft1":
        s, x, chans = b2a_record()
        return s, x, chans, None, 60
    mode = "NB" if name == "nb-ft2" else "WB"
    s1, _, chans = b1c_case(mode)
    s2, x_iq, _ = track_case("B1C", mode, 12, iq=True)
    s2 = s2.copy(CNoInterval=s1.CNoInterval, numberOfChannels=s1.numberOfChannels)
    if name == "nb-ft2":
        x = x_iq
    else:
        x, _ = packed_record(x_iq)
        s2 = s2.copy(fileType=3)
    x.setflags(write=False)
    return s2, x, chans, mode, 12


RECORDS = ["b2a-ft1", "nb-ft2", "wb-ft3"]


@functools.lru_cache(maxsize=None)
def one_shot(name):
    """tracking() on the host bytes: computed once, shared and left unchanged."""
    s, x, chans, mode, n = track_record(name)
    want, _ = bds_amd.tracking(x, chans, s, mode=mode)
    assert [w.completed for w in want][:2] == [n, n]
    c = bds_amd.get_context(0)
    return want, c.track_stream_info(), c.track_loaded_bytes()


@pytest.mark.parametrize("name", RECORDS)
def test_tracking_a_device_tensor_equals_tracking_host_bytes(ctx, name):
    s, x, chans, mode, _ = track_record(name)
    want, info, loaded = one_shot(name)
    got, _ = bds_amd.tracking(dev(x, 3), chans, s, mode=mode)
    assert_same_results(got, want)
    assert ctx.track_stream_info() == info and ctx.track_loaded_bytes() == loaded and loaded > 0
    # streamed through a small resident span: the loader thread's pieces come from the device too
    limit = 24 * (spc_of(s) * {1: 1, 2: 2, 3: 1}[int(s.fileType)] // (2 if int(s.fileType) == 3 else 1)) if name == "b2a-ft1" else None
    if limit:
        host, _ = bds_amd.tracking(x, chans, s, mode=mode, resident_limit=limit)
        h_info, h_loaded = ctx.track_stream_info(), ctx.track_loaded_bytes()
        got, _ = bds_amd.tracking(dev(x, 1), chans, s, mode=mode, resident_limit=limit)
        assert_same_results(host, want)
        assert_same_results(got, want)
        assert ctx.track_stream_info() == h_info and ctx.track_loaded_bytes() == h_loaded and h_info["pieces"] > 1


def run_session(ctx, source, chans, s, pieces, mode, **kw):
    calls = []
    with bds_amd.TrackSession(source, chans, s, mode=mode, **kw) as t:
        for n in pieces:
            calls.append(t.advance(n))
            assert t.last_k == n
        info = t.info()
        stream, loaded = ctx.track_stream_info(), ctx.track_loaded_bytes()
    return calls, info, stream, loaded


def assert_same_info(a, b):
    assert sorted(a) == sorted(b)
    for k, v in a.items():
        np.testing.assert_array_equal(v, b[k], err_msg=k)


@pytest.mark.parametrize("name", RECORDS)
def test_a_session_on_a_device_tensor_equals_the_host_session(ctx, name):
    s, x, chans, mode, n = track_record(name)
    d = dev(x, 5)
    for pieces in PIECES[n]:
        want = run_session(ctx, x, chans, s, pieces, mode)
        got = run_session(ctx, d, chans, s, pieces, mode)
        for a, b in zip(got[0], want[0]):
            assert_same_results(a, b)
        assert_same_info(got[1], want[1])
        assert got[2] == want[2] and got[3] == want[3] and want[3] > 0
    if name == "b2a-ft1":  # a moving span: several pieces within an advance and across advances, the loader thread at work
        limit = 24 * spc_of(s)
        want = run_session(ctx, x, chans, s, PIECES[n][0], mode, resident_limit=limit)
        got = run_session(ctx, d, chans, s, PIECES[n][0], mode, resident_limit=limit)
        for a, b in zip(got[0], want[0]):
            assert_same_results(a, b)
        assert got[2] == want[2] and got[3] == want[3] and want[2]["pieces"] > 2


def minimum_limit(chans, s, origin=0):
    with pytest.raises(native.BdsError) as ei:
        bds_amd.TrackSession(None, chans, s, origin=origin, resident_limit=1)
    m = re.search(r"at least (\d+) bytes", str(ei.value))
    assert m, str(ei.value)
    return int(m.group(1))


def feed_all(ctx, t, chunks, n_adv):
    """Feed the chunks in order (the last with last=True), one advance(n_adv) after every feed call; then advance until nothing runs
    any more.  Returns (the calls that ran epochs, the bytes taken by each feed call, session info, stream info, loaded bytes)."""
    calls, took_all = [], []
    for i, piece in enumerate(chunks):
        is_last = i == len(chunks) - 1
        while True:
            size = int(piece.numel()) if isinstance(piece, torch.Tensor) else piece.size
            took = t.feed(piece, last=is_last)
            assert 0 <= took <= size
            took_all.append(took)
            r = t.advance(n_adv)
            if t.last_k:
                calls.append(r)
            assert took or t.last_k, "neither a byte taken nor an epoch run: the session is stuck"
            piece = piece[took:]
            if took == size:
                break
    for _ in range(8):
        r = t.advance(n_adv)
        if not t.last_k:
            break
        calls.append(r)
    assert t.last_k == 0
    return calls, took_all, t.info(), ctx.track_stream_info(), ctx.track_loaded_bytes()


def chunks_of(x, file_type):
    """(host chunks, the same chunks as slices of ONE device tensor, each starting at an odd byte offset): FEED_CHUNK bytes each,
    rounded down to whole pairs for an I/Q record."""
    chunk = FEED_CHUNK - FEED_CHUNK % 2 if file_type == 2 else FEED_CHUNK
    stride = chunk + chunk % 2  # (an even stride from offset 1: every slice starts on an odd byte)
    host = [x[o:o + chunk] for o in range(0, x.size, chunk)]
    big = torch.zeros(1 + stride * len(host), dtype=torch.uint8, device=GPU)
    out = []
    for k, h in enumerate(host):
        o = 1 + k * stride
        big[o:o + h.size] = torch.from_numpy(np.array(h, copy=True).view(np.uint8))
        t = big[o:o + h.size]
        assert t.data_ptr() % 2 == 1
        out.append(t.view(torch.int8) if x.dtype == np.int8 else t)
    return host, out


def assert_same_fed_runs(got, want):
    assert got[1] == want[1]  # the same numbers of bytes taken at the same calls
    assert len(got[0]) == len(want[0]) > 0
    for a, b in zip(got[0], want[0]):
        assert_same_results(a, b)
    assert_same_info(got[2], want[2])
    assert got[3] == want[3] and got[4] == want[4] and want[4] > 0


@pytest.mark.parametrize("name", RECORDS)
def test_a_feed_session_fed_from_device_slices_equals_the_host_fed_session(ctx, name):
    s, x, chans, mode, n = track_record(name)
    host, device = chunks_of(x, int(s.fileType))
    with bds_amd.TrackSession(None, chans, s, origin=0, mode=mode) as t:
        want = feed_all(ctx, t, host, FEED_ADVANCE)
    with bds_amd.TrackSession(None, chans, s, origin=0, mode=mode) as t:
        got = feed_all(ctx, t, device, FEED_ADVANCE)
    assert_same_fed_runs(got, want)
    assert sum(want[1]) == x.size and sum(r[0].completed for r in want[0]) >= n


def test_feeds_taken_in_part_at_the_minimum_resident_limit(ctx):
    s, x, chans, mode, _ = track_record("b2a-ft1")
    minimum = minimum_limit(chans, s)
    host, device = chunks_of(x, 1)
    with bds_amd.TrackSession(None, chans, s, origin=0, resident_limit=minimum) as t:
        want = feed_all(ctx, t, host, FEED_ADVANCE)
    with bds_amd.TrackSession(None, chans, s, origin=0, resident_limit=minimum) as t:
        got = feed_all(ctx, t, device, FEED_ADVANCE)
        with pytest.raises(native.BdsError, match="end of the record"):
            t.feed(device[0][:16])
    assert_same_fed_runs(got, want)
    assert len(want[1]) > len(host)  # feeds were taken in part
    assert want[3]["resident_max_bytes"] <= minimum and want[3]["repeated_batches"] == 0


# ---- 4. the chain in HBM ---------------------------------------------------------------------------------------------------
def _joined(calls, n_ch):
    out = []
    for c in range(n_ch):
        r = TrackResults()
        for f, v in vars(calls[0][c]).items():
            if isinstance(v, np.ndarray):
                setattr(r, f, np.concatenate([getattr(call[c], f) for call in calls]))
        r.PRN = calls[0][c].PRN
        r.completed = sum(call[c].completed for call in calls)
        out.append(r)
    return out


def _chain(ctx, s, record, n_acq, chunk):
    """acquisition on the first n_acq samples, preRun, a feed session fed with `record` in chunks: (acqResults, channel, results)."""
    acq = bds_amd.acquisition(record[:n_acq], s, verbose=False)
    chans = bds_amd.pre_run(acq, s)
    size = int(record.numel()) if isinstance(record, torch.Tensor) else record.size
    with bds_amd.TrackSession(None, chans, s, origin=0) as t:
        calls, took, info, _, _ = feed_all(ctx, t, [record[o:o + chunk] for o in range(0, size, chunk)], FEED_ADVANCE)
    return acq, chans, _joined(calls, len(chans)), took, info


def test_generate_acquire_and_track_without_leaving_hbm(ctx):
    """A 40-ms B2a record made by make_if_device(out="torch") -- two satellites, Doppler off the 400-Hz grid, code Doppler on -- is
    searched on a device slice and tracked by a session fed from the same tensor; the chain run from tensor.cpu().numpy() gives the
    same bits, and the first 20 epochs are the float64 oracle's at the tolerances of test_b2a_session_against_the_oracle."""
    s = bds_amd.init_settings_b2a(acqSatelliteList=[19, 20], acqSearchBand=800, acqStep=400, fineNoncoh=7, numberOfChannels=2,
                                  CNoInterval=CNO_INTERVAL[60], msToProcess=20)
    spc = spc_of(s)
    sats = [synth.Sat(19, 310.0, 0.37 * spc, 1.1, 47.0), synth.Sat(20, -537.0, 0.71 * spc, 0.3, 46.0)]
    assert all(sat.doppler % 400 for sat in sats)
    t = synth.make_if_device(s, sats, 40 * spc, seed=SEED, code_doppler=True, out="torch")
    assert t.is_cuda and t.dtype == torch.int8 and t.numel() == 40 * spc
    x = t.cpu().numpy()
    got = _chain(ctx, s, t, 10 * spc, FEED_CHUNK)
    want = _chain(ctx, s, x, 10 * spc, FEED_CHUNK)
    for f in ("carrFreq", "codePhase", "peakMetric"):
        np.testing.assert_array_equal(getattr(got[0], f), getattr(want[0], f), err_msg=f)
    assert got[0].carrFreq[18] != 0 and got[0].carrFreq[19] != 0
    assert [vars(c) for c in got[1]] == [vars(c) for c in want[1]] and sorted(c.PRN for c in got[1]) == [19, 20]
    assert got[3] == want[3]
    assert_same_results(got[2], want[2])
    assert_same_info(got[4], want[4])
    assert min(r.completed for r in got[2]) >= 37
    # the first 20 epochs against the oracle on those bytes
    ref, _ = otrk.tracking(otrk.RawFile(x), got[1], s)
    first = []
    for r in got[2]:
        q = TrackResults()
        for f, v in vars(r).items():
            setattr(q, f, (v[: 20 // CNO_INTERVAL[60]] if f in CNO_FIELDS else v[:20]) if isinstance(v, np.ndarray) else v)
        q.status = "T"  # (20 of its epochs, all run: counted above)
        first.append(q)
    assert_closed_loop_parity(ref, first, "B2A")


def test_acquire_track_takes_record_bytes_of_either_kind(ctx, cfg1):
    """acquire_track(long_signal, record): `record` as raw bytes, host or device, goes through the search, bds_pre_run_device and
    bds_track_mem / bds_track_dev, and equals the one-call path on the record's file."""
    s0, x, chans, _, _ = track_record("b2a-ft1")
    s = s0.copy(acqSatelliteList=[19, 20, 33], acqSearchBand=1600, acqStep=400, fineNoncoh=7, numberOfChannels=4, msToProcess=20)
    block = x[: 10 * spc_of(s)]
    want = bds_amd.acquire_track(block, x, s)
    got = bds_amd.acquire_track(dev(block, 1), dev(x, 3), s)
    for f in ("carrFreq", "codePhase", "peakMetric"):
        np.testing.assert_array_equal(getattr(got[0], f), getattr(want[0], f), err_msg=f)
    assert [vars(c) for c in got[1]] == [vars(c) for c in want[1]]
    assert sorted(c.PRN for c in want[1]) == [0, 19, 20, 33]
    assert_same_results(got[2], want[2])
    assert [r.completed for r in want[2] if r.PRN] == [20, 20, 20]


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------
def test_refused_pointers_return_err_arg_and_leave_the_context_working(ctx, cfg1):
    s, x, chans, mode, _ = track_record("b2a-ft1")
    want, _, _ = one_shot("b2a-ft1")
    sa, xa, _ = cfg1
    lib, cs = ctx._lib, native.pack_settings(sa)
    host = np.array(x[:4096], copy=True)
    host_ptr = host.ctypes.data
    small = torch.zeros(4096, dtype=torch.int8, device=GPU)

    def err():
        return lib.bds_last_error(ctx._h).decode()

    # acquisition: a host pointer, a range past the allocation, NULL
    assert lib.bds_acq_load_dev(ctx._h, C.byref(cs), host_ptr, host.size, 0) == -1
    assert "d_samples" in err() and "not device memory" in err()
    assert lib.bds_acq_load_dev(ctx._h, C.byref(cs), small.data_ptr(), 2 ** 40, 0) == -1
    assert "d_samples" in err() and "past its allocation" in err()
    assert lib.bds_acq_load_dev(ctx._h, C.byref(cs), None, 4096, 0) == -1
    assert "d_samples" in err() and "NULL" in err()
    with pytest.raises(native.BdsError, match="d_samples.*not device memory") as ei:
        ctx.acq_load(sa, RawSpan(host_ptr, host.size, owner=host))
    assert ei.value.code == -1
    # tracking, one shot and open
    with pytest.raises(native.BdsError, match="d_file_bytes.*not device memory") as ei:
        bds_amd.tracking(RawSpan(host_ptr, host.size, owner=host), chans, s)
    assert ei.value.code == -1
    with pytest.raises(native.BdsError, match="d_file_bytes.*past its allocation"):
        bds_amd.tracking(RawSpan(small.data_ptr(), 2 ** 40, owner=small), chans, s)
    with pytest.raises(native.BdsError, match="d_file_bytes.*not device memory"):
        bds_amd.TrackSession(RawSpan(host_ptr, host.size, owner=host), chans, s)
    with pytest.raises(native.BdsError, match="d_out.*not device memory"):
        ctx.synth_dev(sa, [], 0, 4096, 1, RawSpan(host_ptr, host.size, owner=host))
    # a feed session: the same three, then the session still takes the record and tracks it
    with bds_amd.TrackSession(None, chans, s, origin=0) as t:
        h = t._sess["handle"]
        assert lib.bds_track_feed_dev(h, host_ptr, host.size, 0) == -1
        assert "d_bytes" in err() and "not device memory" in err()
        assert lib.bds_track_feed_dev(h, small.data_ptr(), 2 ** 40, 0) == -1
        assert "d_bytes" in err() and "past its allocation" in err()
        assert lib.bds_track_feed_dev(h, None, 64, 0) == -1
        assert "d_bytes" in err() and "NULL" in err()
        with pytest.raises(native.BdsError, match="d_bytes.*not device memory") as ei:
            ctx.track_feed_dev(t._sess, RawSpan(host_ptr, host.size, owner=host))
        assert ei.value.code == -1
        assert t.info()["fed_end"] == 0 and t.info()["resident_bytes"] == 0  # nothing was copied
        assert t.feed(dev(x, 1), last=True) == x.size
        got = t.advance(60)
        assert t.last_k == 60
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g.I_P, w.I_P)
        np.testing.assert_array_equal(g.carrFreq, w.carrFreq)
    # feed_dev on a session that reads its record itself, and on a closed one
    with bds_amd.TrackSession(dev(x), chans, s) as t:
        h = t._sess["handle"]
        assert lib.bds_track_feed_dev(h, small.data_ptr(), 64, 0) == -1
        assert "bds_track_feed_dev" in err() and "reads its record itself" in err()
        with pytest.raises(ValueError, match="reads its record itself"):
            t.feed(small[:64])
        first = t.advance(3)
        assert t.last_k == 3
    assert lib.bds_track_feed_dev(h, small.data_ptr(), 64, 0) == -1  # closed: the handle is not read
    with pytest.raises(native.BdsError, match="closed"):
        t.feed(small[:64])
    np.testing.assert_array_equal(first[0].I_P, want[0].I_P[:3])
    # the context still serves the host path, with the results of before
    got, _ = bds_amd.tracking(x, chans, s)
    assert_same_results(got, want)
    acq = bds_amd.acquisition(xa, sa, verbose=False)
    assert acq.carrFreq[18] != 0
