"""bds_corr_function* on the GPU (csrc/bds_corrfn.hip) against the float64 model of tests/corrfn_cases.py, the open-loop test aid and
the trackers; record edges, the five record formats, the determinism contract (bit equality across call composition, batching and
record source) and the argument checks.

Tolerance: the project's open-loop one (tests/test_track_gpu.py) -- every I and Q of an item within
1e-6 |P| of the model, |P| the model's data-component magnitude at tau = 0 of that item.

Measured on an MI355X (worst |error| / |P| over all items, components and taps; profiles/corrfn_errors.txt): see that file."""
import ctypes as C
import functools

import numpy as np
import pytest

import bds_amd
from bds_amd import native

import corrfn_cases as cc
from helpers import track_case
from int16_cases import embed, settings16
from packed_cases import packed_record

pytestmark = pytest.mark.gpu

SHAPES = {"B2A": ("B2A", 8), "NB": ("B1C", 5), "WB": ("B1C", 5)}


@functools.lru_cache(maxsize=None)
def case(mode, iq=False):
    """helpers.track_case at its own small rate, the oracle's trace, and the items of the tests: first, middle and last epoch of the
    three channels.  The record is read-only."""
    signal, n_epochs = SHAPES[mode]
    s, x, chans, trace, _ = cc.traced(signal, mode, n_epochs, iq=iq)
    x.setflags(write=False)
    rows = [t for t in trace if t["k"] in (1, (n_epochs + 1) // 2, n_epochs)]
    prn, st = cc.states_of(rows, chans)
    assert len(prn) == 9 and st[0, 2] == 0.0 and np.all(st[:, 1] % 2048 != 0)
    assert signal == "B2A" or len(set(st[:, 1])) > 1  # (B2a at 25 MS/s: 25 000 samples every epoch; B1C block lengths differ)
    return s, x, chans, prn, st


@functools.lru_cache(maxsize=None)
def reference(mode, iq=False):
    """The model at the full tap set for the nine items: computed once, shared, never modified."""
    s, x, chans, prn, st = case(mode, iq)
    taps = cc.gpu_taps(s.dllCorrelatorSpacing)
    xs = cc.samples_of(x, s)
    want = np.stack([cc.model(xs, s, mode, p, q, taps) for p, q in zip(prn, st)])
    want.setflags(write=False)
    p_mag = np.abs(want[:, 0, list(taps).index(0.0)])
    return taps, want, p_mag


@pytest.mark.parametrize("mode", ["B2A", "NB", "WB"])
def test_kernel_against_model(ctx, mode):
    s, x, chans, prn, st = case(mode)
    taps, want, p_mag = reference(mode)
    got = ctx.corr_function(s, x, prn, st, taps)
    assert got.shape == want.shape == (9, {"B2A": 2, "NB": 2, "WB": 3}[mode], 46)
    cc.assert_close(got, want, p_mag, f"{mode} kernel against model")


@pytest.mark.parametrize("mode", ["B2A", "NB"])
def test_kernel_against_model_iq_record(ctx, mode):
    s, x, chans, prn, st = case(mode, True)
    taps, want, p_mag = reference(mode, True)
    got = ctx.corr_function(s, x, prn, st, taps)
    cc.assert_close(got, want, p_mag, f"{mode} I/Q kernel against model")


@pytest.mark.parametrize("mode", ["B2A", "NB", "WB"])
def test_tracker_taps_equal_the_open_loop_aid(ctx, mode):
    """tau = (-spc, 0, +spc): the 18 sums of bds_track_correlate, within the same 1e-6 |P|."""
    s, x, chans, prn, st = case(mode)
    spc = s.dllCorrelatorSpacing
    got = ctx.corr_function(s, x, prn, st, [-spc, 0.0, spc])
    sums = ctx.track_correlate(s, x, prn, st).reshape(9, 3, 3, 2)[:, : got.shape[1]]
    want = sums[..., 0] + 1j * sums[..., 1]
    p_mag = np.hypot(sums[:, 0, 1, 0], sums[:, 0, 1, 1])
    cc.assert_close(got, want, p_mag, f"{mode} against bds_track_correlate")


def test_composite_equals_the_wide_band_tracker(ctx):
    """composite=True on the trackers' own results: Pilot_I_E .. Pilot_Q_L of bds_amd.tracking on the same record, at the closed-loop
    tolerance of helpers.assert_closed_loop_parity (1e-4 of the largest |P|)."""
    s, x, chans, _, _ = case("WB")
    res, _ = bds_amd.tracking(x, chans, s, mode="WB")
    spc = s.dllCorrelatorSpacing
    z = bds_amd.corr_function(x, chans, s, res, [-spc, 0.0, spc], composite=True, mode="WB")
    n = len(res[0].I_P)
    assert z.shape == (3 * n, 2, 3)
    for c, r in enumerate(res):
        zc = z[c * n:(c + 1) * n]
        p = np.hypot(r.I_P, r.Q_P).max()
        for j, e in enumerate("EPL"):
            np.testing.assert_allclose(zc[:, 0, j].real, getattr(r, "I_" + e), rtol=0, atol=1e-4 * p)
            np.testing.assert_allclose(zc[:, 0, j].imag, getattr(r, "Q_" + e), rtol=0, atol=1e-4 * p)
            np.testing.assert_allclose(zc[:, 1, j].real, getattr(r, "Pilot_I_" + e), rtol=0, atol=1e-4 * p)
            np.testing.assert_allclose(zc[:, 1, j].imag, getattr(r, "Pilot_Q_" + e), rtol=0, atol=1e-4 * p)


def test_record_edges(ctx):
    """An item at sample 0 and an item whose last sample is the record's last: the record is cut to exactly the items' span, so a
    read past either end would leave the allocation's slack; one sample more is refused and names the item."""
    s, x, chans, prn, st = case("B2A")
    taps, want, p_mag = reference("B2A")
    first, last = int(np.argmin(st[:, 0])), int(np.argmax(st[:, 0] + st[:, 1]))
    lo, hi = int(st[first, 0]), int(st[last, 0] + st[last, 1])
    cut = np.ascontiguousarray(x[lo:hi])
    st2 = st[[first, last]].copy()
    st2[:, 0] -= lo
    assert st2[0, 0] == 0 and st2[1, 0] + st2[1, 1] == cut.size
    got = ctx.corr_function(s, cut, prn[[first, last]], st2, taps)
    cc.assert_close(got, want[[first, last]], p_mag[[first, last]], "record edges")
    st3 = st2.copy()
    st3[1, 1] += 1
    with pytest.raises(native.BdsError, match="item 1 reaches past the end of the record"):
        ctx.corr_function(s, cut, prn[[first, last]], st3, taps)


def test_odd_start_sample_in_a_packed_record(ctx):
    s, x, chans, prn, st = case("B2A", True)
    shift = int(st[:, 0].min()) - 33  # the first item then starts at sample 33: the high nibble of byte 16
    packed, pairs = packed_record(x[2 * shift:])
    st2 = st.copy()
    st2[:, 0] -= shift
    assert int(st2[:, 0].min()) == 33
    n = packed.size * 2
    keep = st2[:, 0] + st2[:, 1] <= n
    s3 = s.copy(fileType=3)
    taps = cc.gpu_taps(s.dllCorrelatorSpacing)[:16]
    got = ctx.corr_function(s3, packed, prn[keep], st2[keep], taps)
    xs = cc.samples_of(pairs, s)
    want = np.stack([cc.model(xs, s, "B2A", p, q, taps) for p, q in zip(prn[keep], st2[keep])])
    p_mag = np.abs(np.stack([cc.model(xs, s, "B2A", p, q, [0.0]) for p, q in zip(prn[keep], st2[keep])])[:, 0, 0])
    cc.assert_close(got, want, p_mag, "packed record, odd start")
    same = ctx.corr_function(s, pairs, prn[keep], st2[keep], taps)  # the int8 I/Q record the bytes unpack to: the same floats
    np.testing.assert_array_equal(got, same)


@pytest.mark.parametrize("mode,iq", [("B2A", False), ("NB", True), ("WB", False)])
def test_int16_record_equals_int8_widened(ctx, mode, iq):
    s, x, chans, prn, st = case(mode, iq)
    taps = cc.gpu_taps(s.dllCorrelatorSpacing)[3:12]
    a = ctx.corr_function(s, x, prn, st, taps)
    b = ctx.corr_function(settings16(s), embed(x), prn, st, taps)
    np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("mode", ["B2A", "WB"])
def test_iq_record_with_zero_q_equals_real(ctx, mode):
    s, x, chans, prn, st = case(mode)
    taps = cc.gpu_taps(s.dllCorrelatorSpacing)[3:12]
    a = ctx.corr_function(s, x, prn, st, taps)
    pairs = np.zeros(2 * x.size, dtype=np.int8)
    pairs[0::2] = x
    b = ctx.corr_function(s.copy(fileType=2), pairs, prn, st, taps)
    np.testing.assert_array_equal(a, b)
    c = ctx.corr_function(settings16(s.copy(fileType=2)), embed(pairs), prn, st, taps)
    np.testing.assert_array_equal(a, c)


@pytest.mark.parametrize("mode", ["B2A", "WB"])
def test_result_depends_on_the_item_alone(ctx, mode, tmp_path):
    """Bit equality: each item alone against all together (in another order too); path against host bytes against device tensor; a
    resident limit that forces at least three batches against none.  One item larger than the limit is refused."""
    import torch

    s, x, chans, prn, st = case(mode)
    taps = cc.gpu_taps(s.dllCorrelatorSpacing)
    together = ctx.corr_function(s, x, prn, st, taps)
    for i in (0, 4, 8):
        np.testing.assert_array_equal(ctx.corr_function(s, x, prn[i:i + 1], st[i:i + 1], taps)[0], together[i])
    perm = np.array([5, 2, 8, 0, 7, 1, 3, 6, 4])
    np.testing.assert_array_equal(ctx.corr_function(s, x, prn[perm], st[perm], taps), together[perm])
    path = tmp_path / "record.bin"
    x.tofile(path)
    np.testing.assert_array_equal(ctx.corr_function(s, str(path), prn, st, taps), together)
    np.testing.assert_array_equal(ctx.corr_function(s, torch.from_numpy(x.copy()).cuda(), prn, st, taps), together)
    before = ctx.track_resident_limit()
    blk = int(st[:, 1].max())
    try:
        ctx.track_set_resident_limit(blk + 4096)  # (real int8 record: a byte per sample) one epoch and a little more
        for source in (x, str(path)):
            np.testing.assert_array_equal(ctx.corr_function(s, source, prn, st, taps), together)
            assert ctx.timing()["n_pairs"] >= 3
        ctx.track_set_resident_limit(blk // 2)
        with pytest.raises(native.BdsError, match=r"alone needs \d+ bytes"):
            ctx.corr_function(s, x, prn, st, taps)
    finally:
        ctx.track_set_resident_limit(before)
    np.testing.assert_array_equal(ctx.corr_function(s, x, prn, st, taps), together)
    assert ctx.timing()["n_pairs"] == 1


def _raw_call(ctx, s, x, prn, st, taps, fill=-77.0):
    """The _mem entry straight through ctypes with a pre-filled output: (return code, output)."""
    cs = native.pack_settings(s)
    a, _ = native.record_bytes(s, x)
    prn = np.ascontiguousarray(prn, dtype=np.int32)
    st = np.ascontiguousarray(st, dtype=np.float64)
    tp = np.ascontiguousarray(taps, dtype=np.float64)
    out = np.full(prn.size * 3 * max(tp.size, 1) * 2, fill)
    n_comp = C.c_int32(-5)
    rc = native.lib().bds_corr_function_mem(ctx._h, C.byref(cs), a.ctypes.data_as(C.POINTER(C.c_int8)), a.size, prn.size,
                                            prn.ctypes.data_as(C.POINTER(C.c_int32)), st.ctypes.data_as(C.POINTER(C.c_double)), tp.size,
                                            tp.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n_comp))
    return rc, out, n_comp.value


def test_argument_checks_write_nothing(ctx):
    s, x, chans, prn, st = case("B2A")
    bad_prn = prn.copy()
    bad_prn[3] = 64
    cases = {"no taps": (prn, st, []), "129 taps": (prn, st, np.linspace(-1, 1, 129)), "tau > 16": (prn, st, [0.0, 16.5]),
             "tau < -16": (prn, st, [-16.001]), "NaN tap": (prn, st, [0.0, np.nan]), "inf tap": (prn, st, [np.inf]),
             "PRN 64": (bad_prn, st, [0.0]), "PRN 0": (np.zeros_like(prn), st, [0.0])}
    for what, (p, q, taps) in cases.items():
        rc, out, n_comp = _raw_call(ctx, s, x, p, q, taps)
        assert rc == -1, what  # BDS_ERR_ARG
        assert np.all(out == -77.0) and n_comp == -5, what
    rc, out, n_comp = _raw_call(ctx, s, x, prn, st, np.linspace(-1, 1, 128))  # the limits themselves pass
    assert rc == 0 and n_comp == 2 and not np.any(out[: 9 * 2 * 128 * 2] == -77.0)
    rc, out, n_comp = _raw_call(ctx, s, x, prn, st, [-16.0, 16.0])
    assert rc == 0
    frac = st.copy()
    frac[1, 0] += 0.5
    assert _raw_call(ctx, s, x, prn, frac, [0.0])[0] == -1


def test_refused_beside_an_open_tracking_session(ctx):
    """The entries share the context's code tables with the trackers: beside an open session they are refused, as tracking() is."""
    s, x, chans, prn, st = case("B2A")
    want = ctx.corr_function(s, x, prn[:2], st[:2], [0.0])
    with bds_amd.TrackSession(x, chans, s, ctx=ctx):
        with pytest.raises(native.BdsError, match="open tracking session"):
            ctx.corr_function(s, x, prn[:2], st[:2], [0.0])
    np.testing.assert_array_equal(ctx.corr_function(s, x, prn[:2], st[:2], [0.0]), want)


@pytest.mark.parametrize("fs,IF", [(3.1e6, 0.8e6), (1.5e6, 0.4e6)])
def test_wide_band_below_the_boc61_rate(ctx, fs, IF):
    """bds_track_correlate accepts wide-band mode below 12.276 MS/s, where a sample step skips BOC(6,1) units (several index steps
    share one first sample); at 1.5 MS/s a chunk also spans more code units than the LDS slice holds, so look-ups go to global
    memory.  First-epoch states of the three channels and a second block with non-zero phases, against the model."""
    s, x, chans = track_case("B1C", "WB", 3, fs=fs, IF=IF)
    prn, st = [], []
    for ch in chans:
        blk = float(int(np.ceil(s.codeLength / (ch.codeFreq / fs))))
        pos = float((int(ch.codePhase) - 1) % int(blk))  # (track_case's delays are those of its 12.5 MS/s record: the first code start inside this one)
        prn += [ch.PRN, ch.PRN]
        st.append([pos, blk, 0.0, ch.codeFreq, 0.0, ch.acquiredFreq])
        rem = 0.37
        st.append([pos + blk, float(int(np.ceil((s.codeLength - rem) / (ch.codeFreq / fs)))), rem, ch.codeFreq, 1.1, ch.acquiredFreq + 3.0])
    prn, st = np.array(prn, dtype=np.int32), np.array(st)
    taps = cc.gpu_taps(s.dllCorrelatorSpacing)
    xs = cc.samples_of(x, s)
    want = np.stack([cc.model(xs, s, "WB", p, q, taps) for p, q in zip(prn, st)])
    p_mag = np.abs(want[:, 0, list(taps).index(0.0)])
    got = ctx.corr_function(s, x, prn, st, taps)
    cc.assert_close(got, want, p_mag, f"WB at {fs / 1e6} MS/s against model")
    sums = ctx.track_correlate(s, x, prn, st).reshape(len(prn), 3, 3, 2)
    spc = s.dllCorrelatorSpacing
    three = ctx.corr_function(s, x, prn, st, [-spc, 0.0, spc])
    cc.assert_close(three, sums[..., 0] + 1j * sums[..., 1], p_mag, f"WB at {fs / 1e6} MS/s against bds_track_correlate")
