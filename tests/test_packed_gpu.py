"""Packed 2+2-bit I/Q records (settings.fileType 3, is_complex 2; the input of B2a/include/unpack_cplx.m:18-30) on the GPU.

The whole specification is one sentence: for packed bytes P, every output of every entry with fileType 3 (is_complex 2) on P equals,
bit for bit, the output of the same call with fileType 2 (is_complex 1) on unpack_cplx(P).  So every comparison below is
assert_array_equal against the fileType-2 run on the unpacked bytes, on the same context -- no tolerance anywhere; the one
comparison with a tolerance is the oracle's, once, on the unpacked record.

Shapes: the reduced-rate ones of tests/helpers.py (B2a at 25 MS/s, spc = 25 000; B1C at 12.5 MS/s, spc = 125 000), quantised to
the alphabet {+-1, +-3} by tests/packed_cases.py."""
import contextlib
import functools

import numpy as np
import pytest

import bds_amd
from bds_amd import native, synth
from oracle import tracking as otrk
from oracle import unpack as oun

from helpers import as_complex, assert_closed_loop_parity, cfg1_b2a_iq, small_b1c_iq, spc_of, track_case
from packed_cases import packed_record

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


@contextlib.contextmanager
def tuned(ctx, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx.reload_tuning()
    try:
        yield
    finally:
        for k in env:
            monkeypatch.delenv(k)
        ctx.reload_tuning()


N_EPOCHS = {"B2A": 60, "NB": 8, "WB": 12}


@functools.lru_cache(maxsize=None)
def record(mode):
    """(fileType-2 settings, fileType-3 settings, packed bytes P, unpack_cplx(P), channels) of a tracking case; the start samples
    skipNumberOfBytes + codePhase - 1 of the channels are of both parities (an odd one starts on a high nibble):
    B2a -- one sample of junk in front and skipNumberOfBytes = 1 make all three odd, and the channels' code Doppler (up to 47
    samples / s) moves them over even ones within the 60 epochs; B1C -- channel 1 starts one sample (0.08 chip) late."""
    signal = "B2A" if mode == "B2A" else "B1C"
    s2, x, chans = track_case(signal, mode, N_EPOCHS[mode], iq=True)
    if mode == "B2A":
        x = np.concatenate([np.array([-35, 7], dtype=np.int8), x])
        s2 = s2.copy(skipNumberOfBytes=1)
    else:
        chans[1].codePhase += 1.0
    packed, pairs = packed_record(x)
    starts = [int(s2.skipNumberOfBytes) + int(c.codePhase) - 1 for c in chans]
    assert {p % 2 for p in starts} == ({1} if mode == "B2A" else {0, 1}), starts
    packed.setflags(write=False), pairs.setflags(write=False)
    return s2, s2.copy(fileType=3), packed, pairs, chans


@functools.lru_cache(maxsize=None)
def tracked(mode):
    """One-window trackResults of the fileType-2 run on the unpacked record, and the bytes it loaded: computed once."""
    s2, _, _, pairs, chans = record(mode)
    ctx = bds_amd.get_context(0)
    assert ctx.track_resident_limit() == 0
    want, _ = bds_amd.tracking(pairs, chans, s2, mode=mode)
    assert ctx.track_stream_info()["pieces"] == 1
    return want, ctx.track_loaded_bytes()


def packed_unit(s):
    """Bytes of one code period of a packed record."""
    return spc_of(s) // 2


# ---- open loop: every alignment ------------------------------------------------------------------------------------------
VARIANTS = [(f"prec{p}-seg{g}", {"BDS_TRK_PREC": str(p), "BDS_TRK_SEG": str(g)}) for p in range(6) for g in (8, 16)]
VARIANTS.append(("per-sample", {"BDS_TRK_PERSAMPLE": "1"}))


@functools.lru_cache(maxsize=None)
def open_loop_states(mode):
    """27 channels: start samples 0 .. 8 (the eight (byte mod 4, nibble) alignments of a lane's first dword and the wrap) x
    blksize nominal, nominal - 1 (odd / even ends, a partial last segment) and 37 (one partial pass)."""
    s2, _, _, _, chans = record(mode)
    step = s2.codeFreqBasis / s2.samplingFreq
    prn, st = [], []
    for start in range(9):
        for j, short in enumerate((0, 1, None)):
            rem = 0.137 * (start + 1)
            nominal = int(np.ceil((s2.codeLength - rem) / step))
            blk = 37 if short is None else nominal - short
            c = chans[(start + j) % len(chans)]
            prn.append(c.PRN)
            st.append([start, blk, rem, c.codeFreq, 0.3 + 0.5 * start, c.acquiredFreq])
    return prn, st


@pytest.mark.parametrize("variant,env", VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize("mode", ["B2A", "NB", "WB"])
def test_open_loop_every_alignment(ctx, monkeypatch, mode, variant, env):
    s2, s3, packed, pairs, _ = record(mode)
    prn, st = open_loop_states(mode)
    with tuned(ctx, monkeypatch, env):
        want = ctx.track_correlate(s2, pairs, prn, st)
        got = ctx.track_correlate(s3, packed, prn, st)
    assert np.all(np.any(want[:, :6] != 0, axis=1))  # every channel correlated something
    np.testing.assert_array_equal(got, want)  # all 18 sums of all 27 channels


# ---- closed loop ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["B2A", "NB", "WB"])
def test_closed_loop_from_memory_and_from_a_file(ctx, tmp_path, mode):
    _, s3, packed, _, chans = record(mode)
    want, _ = tracked(mode)
    assert all(w.status == "T" and w.completed == N_EPOCHS[mode] for w in want)
    parities = {int(a) % 2 for w in want for a in w.absoluteSample}
    assert parities == {0, 1}  # epochs start on low and on high nibbles
    path = tmp_path / "packed.bin"
    packed.tofile(path)
    for source in (packed, str(path), packed.view(np.int8)):  # (raw file bytes as int8 are the same bytes)
        got, _ = bds_amd.tracking(source, chans, s3, mode=mode)
        assert ctx.track_stream_info()["pieces"] == 1
        assert_same_results(got, want)  # every field, C/N0 and lock detector included


def test_closed_loop_against_the_oracle(ctx):
    s2, s3, packed, pairs, chans = record("WB")
    ref, _ = otrk.tracking(otrk.RawFile(np.asarray(pairs)), chans, s2, mode="WB")
    got, _ = bds_amd.tracking(packed, chans, s3, mode="WB")
    assert_closed_loop_parity(ref, got, "WB")


# ---- streamed ------------------------------------------------------------------------------------------------------------
# the limits of tests/test_track_stream_gpu.py in code periods of PACKED bytes; the last one is no multiple of 16 bytes
B2A_LIMITS = [(12.0, 0, 5), (7.5, 0, 8), (5.0, 0, 12), (7.5, 7, 8)]


@pytest.mark.parametrize("periods,odd,min_pieces", B2A_LIMITS)
def test_b2a_streamed(ctx, tmp_path, periods, odd, min_pieces):
    _, s3, packed, _, chans = record("B2A")
    want, _ = tracked("B2A")
    one_window, _ = bds_amd.tracking(packed, chans, s3, mode="B2A")
    limit = int(periods * packed_unit(s3)) + odd
    path = tmp_path / "packed.bin"
    packed.tofile(path)
    for source in (packed, str(path)):
        got, _ = bds_amd.tracking(source, chans, s3, mode="B2A", resident_limit=limit)
        info = ctx.track_stream_info()
        assert info["pieces"] >= min_pieces, info
        assert 0 < info["resident_max_bytes"] <= limit, info
        assert info["repeated_batches"] == 0, info
        assert_same_results(got, one_window)
        assert_same_results(got, want)
    assert ctx.track_resident_limit() == 0


@pytest.mark.parametrize("mode", ["WB", "NB"])
def test_b1c_streamed(ctx, mode):
    _, s3, packed, _, chans = record(mode)
    want, _ = tracked(mode)
    limit = 4 * packed_unit(s3)
    got, _ = bds_amd.tracking(packed, chans, s3, mode=mode, resident_limit=limit)
    info = ctx.track_stream_info()
    assert info["pieces"] >= N_EPOCHS[mode] // 2 and info["resident_max_bytes"] <= limit and info["repeated_batches"] == 0, info
    assert_same_results(got, want)


def test_limit_below_the_minimum_states_packed_bytes(ctx):
    import re

    _, s3, packed, _, chans = record("B2A")
    want, _ = tracked("B2A")
    with pytest.raises(native.BdsError, match="of the packed record") as ei:
        bds_amd.tracking(packed, chans, s3, mode="B2A", resident_limit=2 * packed_unit(s3))
    minimum = int(re.search(r"at least (\d+) bytes", str(ei.value)).group(1))
    # spread of the start samples (17 111) + one block at a code rate 2 % low + what a span start can fall behind, twice,
    # at half a byte per sample
    assert 17111 + 25000 < minimum < 17111 + 1.1 * 25000
    with pytest.raises(native.BdsError):
        bds_amd.tracking(packed, chans, s3, mode="B2A", resident_limit=minimum - 1)
    got, _ = bds_amd.tracking(packed, chans, s3, mode="B2A", resident_limit=minimum)
    assert ctx.track_stream_info()["resident_max_bytes"] <= minimum
    assert_same_results(got, want)


# ---- loaded bytes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["B2A", "WB"])
def test_a_quarter_of_the_bytes_is_loaded(ctx, mode):
    """Both runs load the same sample range; the only slack is alignment: <= 32 samples at each end, so <= 32 bytes."""
    _, s3, packed, _, chans = record(mode)
    _, loaded_iq = tracked(mode)
    bds_amd.tracking(packed, chans, s3, mode=mode)
    loaded = ctx.track_loaded_bytes()
    assert ctx.track_stream_info()["resident_max_bytes"] == loaded
    assert 0 < loaded <= loaded_iq / 4 + 64, (loaded, loaded_iq)
    assert loaded >= loaded_iq // 4


# ---- short file ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drop", [0, 1], ids=["even-bytes", "odd-bytes"])
def test_short_file(ctx, tmp_path, drop):
    """B2a/tracking.m:250-254 in samples: the packed record cut to 25 code periods, and to an odd byte count; one window, and
    streamed with the end of the file in a later piece."""
    s2, s3, packed, _, chans = record("B2A")
    cut = packed[: 25 * packed_unit(s3) - drop]
    assert cut.size % 2 == drop
    want, _ = bds_amd.tracking(oun.unpack_cplx(cut), chans, s2, mode="B2A")
    assert [w.status for w in want] == ["-", "-", "-"] and 0 < want[0].completed < 60
    path = tmp_path / "short.bin"
    cut.tofile(path)
    for source in (cut, str(path)):
        got, _ = bds_amd.tracking(source, chans, s3, mode="B2A")
        assert ctx.track_stream_info()["pieces"] == 1
        assert_same_results(got, want)  # completed, status and the partial results
        got, _ = bds_amd.tracking(source, chans, s3, mode="B2A", resident_limit=8 * packed_unit(s3))
        assert ctx.track_stream_info()["pieces"] >= 5
        assert_same_results(got, want)
        for c in (1, 2):
            assert got[c].completed == 0 and not np.any(got[c].I_P) and np.all(np.isinf(got[c].carrFreq))


# ---- acquisition ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def acq_block(name):
    s2, x, _ = {"b2a": cfg1_b2a_iq, "b1c": small_b1c_iq}[name]()
    packed, pairs = packed_record(x)
    return s2, s2.copy(fileType=3), packed, pairs


def _grid(s, samples, is_complex, n_samples=None):
    """Results, row maxima of the search grid and timing of one load / prepare / run on a context of its own."""
    c = native.Context(0)
    try:
        c.acq_load(s, samples, is_complex, n_samples)
        c.acq_prepare(s)
        res = c.acq_run(s)
        tm = c.timing()
        grid, arg = c.acq_grid(len(s.acqSatelliteList), int(tm["n_bins"]))
    finally:
        c.close()
    return res, grid, arg, tm


def _same_acq(got, want):
    for g, w in zip(got[0], want[0]):  # carrFreq, codePhase, peakMetric, detected
        np.testing.assert_array_equal(g, w)
    np.testing.assert_array_equal(got[1], want[1])  # row maxima
    np.testing.assert_array_equal(got[2], want[2])  # and where they are


@pytest.mark.parametrize("name", ["b2a", "b1c"])
def test_acquisition(ctx, name):
    s2, s3, packed, pairs = acq_block(name)
    want = bds_amd.acquisition(as_complex(pairs), s2, verbose=False)
    got = bds_amd.acquisition(packed, s3, verbose=False)
    assert np.count_nonzero(want.carrFreq) >= 1
    for f in ("carrFreq", "codePhase", "peakMetric"):
        np.testing.assert_array_equal(getattr(got, f), getattr(want, f), err_msg=f)
    _same_acq(_grid(s3, packed, 2), _grid(s2, pairs, 1))


def test_acquisition_of_an_odd_number_of_samples(ctx):
    s2, s3, packed, pairs = acq_block("b2a")
    n = packed.size * 2 - 1
    assert n % 2 == 1
    want = _grid(s2, pairs[: 2 * n], 1)
    _same_acq(_grid(s3, packed, 2, n_samples=n), want)
    junk = packed.copy()
    junk[-1] ^= 0xF0  # the last high nibble is not part of the block
    _same_acq(_grid(s3, junk, 2, n_samples=n), want)
    assert np.count_nonzero(want[0][0]) >= 1


def test_b1c_defaults_take_the_n_point_pair_with_packed_input(ctx):
    """init_settings_b1c() as it stands (53 MS/s): the packed block goes through the N-point pair like the I/Q block."""
    s2 = bds_amd.init_settings_b1c(acqSatelliteList=[7, 8, 23], fileType=2, acqSearchBand=400.0)
    spc = spc_of(s2)
    sats = [synth.Sat(7, -330.0, 0.613 * spc, 0.7, 46.0), synth.Sat(23, 210.0, 0.2 * spc, 2.0, 47.0)]
    packed, pairs = packed_record(synth.make_if(s2, sats, 4 * spc, seed=77, iq_sign=-1))
    got, want = _grid(s2.copy(fileType=3), packed, 2), _grid(s2, pairs, 1)
    for tm in (got[3], want[3]):
        assert (tm["rows_kernel"], tm["cols_kernel"], tm["fft_len"]) == (3, 4, 1060000)
    _same_acq(got, want)
    assert got[0][0][6] != 0 and got[0][0][22] != 0 and got[0][0][7] == 0


def test_acquire_track_from_one_packed_file(ctx, tmp_path):
    """bds_acquire_track: the block and the record are the same packed bytes (two satellites on three channels)."""
    s2 = bds_amd.init_settings_b2a(samplingFreq=25e6, IF=6.5e6, acqSatelliteList=[5, 9, 19, 33], acqSearchBand=2500,
                                   fineNoncoh=5, msToProcess=40, numberOfChannels=3, CNoInterval=20, fileType=2)
    s3 = s2.copy(fileType=3)
    sats = [synth.Sat(9, -1230.0, 12345.6, 2.0, 50.0), synth.Sat(19, 2210.0, 3001.2, 0.4, 47.0)]
    spc = spc_of(s2)
    packed, pairs = packed_record(synth.make_if(s2, sats, 60 * spc, seed=123, iq_sign=-1))
    p3, p2 = tmp_path / "packed.bin", tmp_path / "pairs.bin"
    packed.tofile(p3), pairs.tofile(p2)
    acq2, ch2, trk2 = bds_amd.acquire_track(as_complex(pairs[: 16 * spc]), str(p2), s2)
    loaded_iq = ctx.track_loaded_bytes()
    acq3, ch3, trk3 = bds_amd.acquire_track(packed[: 4 * spc], str(p3), s3)
    assert ctx.track_loaded_bytes() <= loaded_iq / 4 + 64
    _, _, trk3s = bds_amd.acquire_track(packed[: 4 * spc], str(p3), s3, resident_limit=4 * spc)
    assert ctx.track_stream_info()["pieces"] >= 5
    for f in ("carrFreq", "codePhase", "peakMetric"):
        np.testing.assert_array_equal(getattr(acq3, f), getattr(acq2, f))
    key = lambda ch: [(c.PRN, c.codePhase, c.acquiredFreq, c.codeFreq, c.status) for c in ch]  # noqa: E731
    assert key(ch3) == key(ch2) and sorted(c.PRN for c in ch3) == [0, 9, 19]
    assert_same_results(trk3, trk2)
    assert_same_results(trk3s, trk2)
    assert [t.status for t in trk3].count("T") == 2


def test_two_packed_jobs_on_aliased_contexts(ctx, monkeypatch):
    """bds_acquire_multi passes a job's is_complex = 2 through: two packed signals over two contexts on device 0."""
    b2, b3, pb, ub = acq_block("b2a")
    c2, c3, pc, uc = acq_block("b1c")
    want_b = bds_amd.acquisition(as_complex(ub), b2, verbose=False)
    want_c = bds_amd.acquisition(as_complex(uc), c2, verbose=False)
    monkeypatch.setenv("BDS_MULTI_TEST_ALIAS", "1")
    m = native.MultiContext([0, 0])
    try:
        assert m.size() == 2
        (cc, pc_, mc, _), (cb, pb_, mb, _) = m.acquire([(c3, pc, 2), (b3, pb, 2)])
    finally:
        m.close()
    for got, want in (((cc, pc_, mc), want_c), ((cb, pb_, mb), want_b)):
        np.testing.assert_array_equal(got[0], want.carrFreq)
        np.testing.assert_array_equal(got[1], want.codePhase)
        np.testing.assert_array_equal(got[2], want.peakMetric)
    assert np.count_nonzero(want_b.carrFreq) >= 1 and np.count_nonzero(want_c.carrFreq) >= 1


# ---- errors --------------------------------------------------------------------------------------------------------------
def test_errors(ctx):
    s2, s3, packed, _ = acq_block("b2a")
    with pytest.raises(native.BdsError, match=r"longSignal has 2000 samples; acquisition needs at least \d+"):
        bds_amd.acquisition(packed[:1000], s3, verbose=False)
    m = native.MultiContext([0])
    try:
        with pytest.raises(native.BdsError, match="has 2000 samples; acquisition needs at least"):
            m.acquire([(s3, packed[:1000], 2)])
    finally:
        m.close()
    with pytest.raises(native.BdsError, match="is_complex must be 0"):
        ctx._check(ctx._lib.bds_acq_load(ctx._h, native.C.byref(native.pack_settings(s3)), native._i8(packed)[1], packed.size, 3))
    st2, st3, tp, _, chans = record("B2A")
    with pytest.raises(native.BdsError, match=r"fileType must be 1 \(real\), 2 \(I/Q\) or 3"):
        bds_amd.tracking(tp.view(np.int8), chans, st3.copy(fileType=4), mode="B2A")
    prn, st = open_loop_states("B2A")
    with pytest.raises(native.BdsError, match="fileType must be"):
        ctx.track_correlate(st3.copy(fileType=4), tp, prn, st)
