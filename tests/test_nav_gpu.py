"""bds_nav_decode on the GPU against the restatement of tests/nav_cases.py: every output bit-equal -- status, polarity, BCH
maxima, packed bits, every bds_eph field with NaN in the same places, firstSubFrame, TOW -- on the smallest prompt series that can
go wrong; then, per signal, a message put into a synthetic record in HBM, tracked, synchronised, decoded and read back."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

import bds_amd
import nav_cases as nc
from bds_amd import native, synth
from helpers import spc_of

pytestmark = pytest.mark.gpu

B1C = bds_amd.init_settings_b1c(pilotTRKflag=2)
B2A = bds_amd.init_settings_b2a()
ALL_OK = nc.BCH1_OK | nc.BCH2_OK | nc.CRC1_OK | nc.CRC2_OK


def check(ctx, settings, prns, sync, data=None, cap=8):
    """Run the device path on [n_ch, n] prompts and hold it to the restatement, channel by channel; returns both."""
    sig = "B1C" if settings is B1C else "B2A"
    got = ctx.nav_decode(settings, prns, sync, data, cap=cap)
    want = [nc.nav_decode_channel(sig, p, sync[c], None if data is None else data[c]) for c, p in enumerate(prns)]
    assert len(got) == len(want)
    for c, (g, w) in enumerate(zip(got, want)):
        assert g["n_frames"] == len(w["frames"]), c
        assert nc.same_frames(g["frames"], w["frames"][:cap]) is None, (c, nc.same_frames(g["frames"], w["frames"][:cap]))
        assert nc.same_eph(g["eph"], w["eph"]) is None, (c, nc.same_eph(g["eph"], w["eph"]))
        assert g["firstSubFrame"] == w["firstSubFrame"] and g["TOW"] == w["TOW"], (c, g["firstSubFrame"], g["TOW"], w["firstSubFrame"], w["TOW"])
    return got, want


def b1c_channel(rng, prn, n, frames):
    """frames: [(index, symbols, sign)] -> (pilot, data)."""
    pilot = nc.b1c_pilot(rng, n, prn, [f[0] for f in frames])
    data = nc.noise_like(rng, n)
    for i, sym, sign in frames:
        nc.place(data, i, sym, rng, sign)
    return pilot, data


def flipped(sym, at):
    s = sym.copy()
    s[at] = -s[at]
    return s


def test_b1c_last_window_in_range(ctx):
    """n = 1800 exactly, one frame at index 1."""
    rng = np.random.default_rng(11)
    bits, sym = nc.b1c_message(rng, 5, 1)
    pilot, data = b1c_channel(rng, 5, 1800, [(1, sym, 1.0)])
    got, _ = check(ctx, B1C, [5], pilot[None], data[None])
    assert got[0]["frames"][0]["status"] == ALL_OK | nc.ENTERED and got[0]["firstSubFrame"] == 1
    np.testing.assert_array_equal(got[0]["frames"][0]["bits"], bits)


@pytest.fixture(scope="module")
def b1c_seven():
    """n = 3700, frames at 37 and 1837, one case per channel (PRNs differ)."""
    rng = np.random.default_rng(12)
    prns = [3, 12, 27, 40, 41, 58, 63]
    chans, msgs = [], []
    for c, prn in enumerate(prns):
        (b1, s1), (b2, s2) = nc.b1c_message(rng, prn, 1, soh=10), nc.b1c_message(rng, prn, 3, soh=11)
        first = {
            0: (s1, 1.0),                                           # as received
            1: (s1, -1.0),                                          # inverted
            2: (s1, -1.0),                                          # first inverted, second not
            3: (flipped(s1, 7), 1.0),                               # a wrong symbol in 1..21: dropped
            4: (flipped(s1, 40), 1.0),                              # a wrong symbol in 22..72: BCH(51,8) fails
            5: (flipped(s1, nc.symbol_of_nav_bit(14 + 333)), 1.0),  # ... in sub-frame 2's kept half: CRC fails, bits reported
            6: (flipped(s1, 72 + 30 * 36 + 21), 1.0),               # ... in a parity half (row 22, column 31: bit 703 of sub-frame 2)
        }[c]
        second = (s2, -1.0 if c == 1 else 1.0)
        chans.append(b1c_channel(rng, prn, 3700, [(37,) + first, (1837,) + second]))
        msgs.append((b1, b2))
    return prns, np.stack([p for p, _ in chans]), np.stack([d for _, d in chans]), msgs


def test_b1c_polarities_and_single_symbol_errors(ctx, b1c_seven):
    prns, pilot, data, msgs = b1c_seven
    got, _ = check(ctx, B1C, prns, pilot, data)
    st = [[f["status"] for f in g["frames"]] for g in got]
    pol = [[f["polarity"] for f in g["frames"]] for g in got]
    ok = ALL_OK | nc.ENTERED
    assert st == [[ok, ok], [ok, ok], [ok, ok], [0, ok], [nc.BCH1_OK, ok], [ALL_OK & ~nc.CRC1_OK, ok], [ok, ok]]
    assert pol == [[1, 1], [-1, -1], [-1, 1], [0, 1], [1, 1], [1, 1], [1, 1]]
    assert [g["firstSubFrame"] for g in got] == [37, 37, 37, 1837, 1837, 1837, 37]
    assert got[3]["frames"][0]["bch1_max"] < 20 and got[4]["frames"][0]["bch2_max"] == 49
    np.testing.assert_array_equal(got[6]["frames"][0]["bits"], msgs[6][0])
    assert np.count_nonzero(got[5]["frames"][0]["bits"] != msgs[5][0]) == 1


def test_b1c_flag_gate_page_1_then_page_3(ctx, b1c_seven):
    """Frame 1 carries page 1 and SOH 10, frame 2 page 3 and SOH 11: SOH, TOW and sub-frame 2 stay the first frame's, both pages'
    fields are there."""
    prns, pilot, data, msgs = b1c_seven
    got, _ = check(ctx, B1C, prns[:1], pilot[:1], data[:1])
    e = got[0]["eph"]
    assert e["SOH"] == 180 and e["PageID1"] == 1 and e["PageID3"] == 3 and e["n_entered"] == 2
    assert not math.isnan(e["alpha1"]) and not math.isnan(e["A_0BGTO"])
    assert e["TOW"] == e["HOW"] * 3600 + 180 == got[0]["TOW"]


def test_b1c_zero_and_nan_prompts_read_as_bit_0(ctx):
    rng = np.random.default_rng(13)
    bits, sym = nc.b1c_message(rng, 9, 1)
    pilot, data = b1c_channel(rng, 9, 1900, [(60, sym, 1.0)])
    zeros = np.nonzero(sym < 0)[0]  # symbols whose intended bit is 0
    pick = np.concatenate([zeros[zeros < 21][:2], zeros[(zeros >= 21) & (zeros < 72)][:2], zeros[zeros >= 72][:6]])
    data[59 + pick] = np.resize([0.0, np.nan, -0.0], pick.size)
    got, _ = check(ctx, B1C, [9], pilot[None], data[None])
    assert got[0]["frames"][0]["status"] == ALL_OK | nc.ENTERED
    np.testing.assert_array_equal(got[0]["frames"][0]["bits"], bits)


def test_b1c_channel_without_candidates_among_others(ctx, b1c_seven):
    prns, pilot, data, _ = b1c_seven
    rng = np.random.default_rng(14)
    p = np.stack([pilot[0], nc.noise_like(rng, 3700), pilot[2]])
    d = np.stack([data[0], nc.noise_like(rng, 3700), data[2]])
    got, _ = check(ctx, B1C, [prns[0], 30, prns[2]], p, d)
    assert got[1]["n_frames"] == 0 and math.isinf(got[1]["TOW"]) and got[1]["eph"]["flag"] == 0
    assert got[0]["n_frames"] == got[2]["n_frames"] == 2


def test_b1c_cap_smaller_than_the_candidate_count(ctx, b1c_seven):
    prns, pilot, data, _ = b1c_seven
    got, want = check(ctx, B1C, prns, pilot, data, cap=1)
    assert all(len(g["frames"]) == 1 and g["n_frames"] == 2 for g in got)
    assert got[3]["firstSubFrame"] == 1837  # from the frame that was not written
    got0, _ = check(ctx, B1C, prns[:2], pilot[:2], data[:2], cap=0)
    assert got0[0]["frames"] == [] and got0[0]["eph"]["n_entered"] == 2


def test_b2a_window_exact_and_one_short(ctx):
    rng = np.random.default_rng(21)
    bits, sym = nc.b2a_message(rng, 19, 10)
    ip = np.zeros(3000)
    nc.place(ip, 1, sym, rng)
    got, _ = check(ctx, B2A, [19], ip[None])
    assert got[0]["frames"][0]["status"] == nc.CRC1_OK | nc.ENTERED and got[0]["firstSubFrame"] == 1
    np.testing.assert_array_equal(got[0]["frames"][0]["bits"], bits)
    k = 7
    short = np.concatenate([nc.noise_like(rng, k), ip[:2999]])  # the preamble at k + 1, 2999 prompts from there on
    got, _ = check(ctx, B2A, [19], short[None])
    assert [f["status"] for f in got[0]["frames"]] == [nc.SHORT] and got[0]["frames"][0]["index"] == k + 1
    assert math.isinf(got[0]["TOW"]) and math.isinf(got[0]["firstSubFrame"]) and got[0]["eph"]["flag"] == 0


def chips(sym, at):
    """`sym` (3000 one-millisecond symbols) with the chips `at` negated."""
    s = sym.copy()
    s[list(at)] *= -1
    return s


def test_b2a_chip_errors_inversion_and_prn_0(ctx):
    """n = 6200, frames at 45 and 3045, message types 10 / 11 / 30 / 34."""
    rng = np.random.default_rng(22)
    m = {t: nc.b2a_message(rng, 20 + t % 7, t) for t in (10, 11, 30, 34)}
    prn0 = nc.b2a_message(rng, 0, 10)
    plan = [
        [(m[10][1], -1.0), (m[11][1], 1.0)],                              # an inverted frame
        [(chips(m[11][1], (3, 61)), 1.0),                            # two wrong chips in the preamble: 116 > 115 still syncs
         (chips(m[30][1], (5 * 100 + 1, 5 * 100 + 3)), 1.0)],        # two wrong chips in symbol 101: the vote holds
        [(chips(m[30][1], (5 * 200, 5 * 200 + 2, 5 * 200 + 4)), 1.0),  # three: the symbol flips, the CRC fails
         (m[34][1], 1.0)],
        [(prn0[1], 1.0), (m[34][1], 1.0)],                                # CRC-valid with PRN field 0 ahead of a valid one
    ]
    ip = []
    for frames in plan:
        x = nc.noise_like(rng, 6200)
        for at, (sym, sign) in zip((45, 3045), frames):
            nc.place(x, at, sym, rng, sign)
        ip.append(x)
    got, _ = check(ctx, B2A, [19, 20, 21, 22], np.stack(ip))
    ok = nc.CRC1_OK | nc.ENTERED
    assert [[f["status"] for f in g["frames"]] for g in got] == [[ok, ok], [ok, ok], [0, ok], [nc.CRC1_OK | nc.PRN_RANGE, ok]]
    assert [[f["polarity"] for f in g["frames"]] for g in got] == [[-1, 1], [1, 1], [1, 1], [1, 1]]
    assert [g["firstSubFrame"] for g in got] == [45, 45, 3045, 3045]
    np.testing.assert_array_equal(got[1]["frames"][1]["bits"], m[30][0])
    assert list(got[0]["eph"]["idValid"][:2]) == [10, 11] and got[3]["eph"]["n_entered"] == 1
    got1, _ = check(ctx, B2A, [19, 20, 21, 22], np.stack(ip), cap=1)
    assert [g["firstSubFrame"] for g in got1] == [45, 45, 3045, 3045]


def test_host_mirror_over_track_results(ctx, b1c_seven):
    prns, pilot, data, msgs = b1c_seven
    tr = [SimpleNamespace(PRN=prns[0], Pilot_I_P=pilot[0], Pilot_Q_P=data[0] * 0, I_P=data[0]), SimpleNamespace(PRN=0),
          SimpleNamespace(PRN=None), SimpleNamespace(PRN=prns[2], Pilot_I_P=pilot[2], Pilot_Q_P=data[2] * 0, I_P=data[2])]
    out = bds_amd.nav_decode(tr, B1C)
    assert len(out) == 2
    want, _ = nc.nav_fields_ref("B1C", list(msgs[0]))
    assert out[0].eph.SOH == want["SOH"] and out[0].eph.omega == want["omega"] and out[0].eph.flag == 1
    assert out[0].firstSubFrame == 37 and out[0].TOW == want["TOW"] and out[0].frames[1].index == 1837
    assert out[0].eph.SatType in ("", "GEO", "IGSO", "MEO") and not hasattr(out[0].eph, "SOW")
    eph, first, tow = bds_amd.BCNAV1decoding(tr, 4, B1C)
    assert first == 37 and tow == out[1].TOW and eph.PRN == prns[2]
    # narrow-band tracking reads Pilot_Q_P (BCNAV1decoding.m:66-73): zeros there, no candidate
    assert bds_amd.nav_decode(tr, B1C.copy(pilotTRKflag=1))[0].n_frames == 0
    rng = np.random.default_rng(31)
    bits, sym = nc.b2a_message(rng, 33, 11)
    ip = nc.noise_like(rng, 3100)
    nc.place(ip, 80, sym, rng, -1.0)
    eph, first, tow = bds_amd.BCNAV2decoding(ip)
    ref, _ = nc.nav_fields_ref("B2A", [bits])
    assert first == 80 and tow == ref["SOW"] and eph.PRN == 33 and eph.C_uc == ref["C_uc"]
    assert eph.t_oe is None and not hasattr(eph, "SOH")


def test_argument_errors_come_before_any_device_call(ctx):
    x = np.ones((1, 1800))
    with pytest.raises(native.BdsError, match="PRN 64 out of range"):
        ctx.nav_decode(B1C, [64], x, x)
    with pytest.raises(native.BdsError, match="data_prompt must be NULL"):
        ctx.nav_decode(B2A, [1], x, x.copy())
    lib, cs = ctx._lib, native.pack_settings(B1C)
    e = native.Eph()  # .size not set
    one = np.zeros(1)
    dp = lambda a: a.ctypes.data_as(native._DP)  # noqa: E731
    prn = np.array([5], dtype=np.int32)
    rc = lib.bds_nav_decode(ctx._h, cs, 1, prn.ctypes.data_as(native._IP), dp(x), None, 1800, None, None, 0, e, dp(one), dp(one.copy()))
    assert rc == -1 and "eph[0].size" in lib.bds_last_error(ctx._h).decode()


# ---- a message in at one end, the same message out at the other -----------------------------------------------------------------------
START = 41  # the frame's first epoch, 1-based: past the loops' transient


def _track(settings, sat, symbols, n_epochs):
    spc = spc_of(settings)
    rec = synth.make_if_device(settings, [sat], (n_epochs + 3) * spc, seed=77, symbols=symbols[None], pilot61_secondary=True, out="torch")
    cf = settings.IF + sat.doppler
    b1c = str(settings.signal).upper() == "B1C"
    code_freq = settings.codeFreqBasis - (cf - settings.IF) / settings.carrFreqBasis * settings.codeFreqBasis if b1c else settings.codeFreqBasis
    chan = SimpleNamespace(PRN=sat.prn, acquiredFreq=float(cf), codePhase=float(int(np.ceil(sat.delay)) + 1), codeFreq=float(code_freq),
                           status="T")
    res, _ = bds_amd.tracking(rec, [chan], settings)
    assert res[0].status == "T" and res[0].completed == n_epochs
    return res


def _symbol_rows(rng, n_sym, data, secondary=None):
    """int8 [2, n_sym]: code period p reads index (p + 1) mod n_sym, so epoch START (1-based) reads index START."""
    rows = rng.choice(np.array([-1, 1], dtype=np.int8), (2, n_sym))
    rows[0, START:START + data.size] = data
    if secondary is not None:
        rows[1, START:START + secondary.size] = secondary
    return rows


def test_b1c_message_end_to_end(ctx):
    """One satellite at 50 dB-Hz, 12.5 MS/s, wide-band tracking over 1850 ten-millisecond epochs."""
    rng = np.random.default_rng(41)
    n_epochs = 1850
    s = bds_amd.init_settings_b1c(samplingFreq=12.5e6, IF=3.5e6, msToProcess=n_epochs * 10, numberOfChannels=1, pilotTRKflag=2,
                                  CNoInterval=50, FEBW=10e6)
    bits, sym = nc.b1c_message(rng, 12, 1, soh=77)
    rows = _symbol_rows(rng, n_epochs + 8, sym, native.gen_code("B1C", "pilot_secondary", 12))
    res = _track(s, synth.Sat(12, -410.0, 0.61, 2.0, 50.0), rows, n_epochs)
    sync = bds_amd.frame_sync(res, s)
    assert list(sync[0][1]) == [START]
    out = bds_amd.nav_decode(res, s)[0]
    assert out.n_frames == 1 and out.frames[0].status == ALL_OK | nc.ENTERED and out.firstSubFrame == START
    np.testing.assert_array_equal(out.frames[0].bits, bits)
    want, _ = nc.nav_fields_ref("B1C", [bits])
    got = ctx.nav_decode(s, [12], np.asarray(res[0].Pilot_I_P)[None], np.asarray(res[0].I_P)[None])[0]
    assert nc.same_eph(got["eph"], want) is None, nc.same_eph(got["eph"], want)
    assert out.TOW == want["TOW"] == want["HOW"] * 3600 + 77 * 18


def test_b2a_message_end_to_end(ctx):
    """One satellite at 50 dB-Hz, 25 MS/s, 3050 one-millisecond epochs."""
    rng = np.random.default_rng(42)
    n_epochs = 3050
    s = bds_amd.init_settings_b2a(samplingFreq=25e6, IF=6.5e6, msToProcess=n_epochs, numberOfChannels=1, CNoInterval=200)
    bits, sym = nc.b2a_message(rng, 19, 10)
    rows = _symbol_rows(rng, n_epochs + 8, sym)
    res = _track(s, synth.Sat(19, -110.0, 0.43, 0.7, 50.0), rows, n_epochs)
    sync = bds_amd.frame_sync(res, s)
    assert list(sync[0][1]) == [START]
    out = bds_amd.nav_decode(res, s)[0]
    assert out.n_frames == 1 and out.frames[0].status == nc.CRC1_OK | nc.ENTERED and out.firstSubFrame == START
    np.testing.assert_array_equal(out.frames[0].bits, bits)
    want, _ = nc.nav_fields_ref("B2A", [bits])
    got = ctx.nav_decode(s, [19], np.asarray(res[0].I_P)[None])[0]
    assert nc.same_eph(got["eph"], want) is None, nc.same_eph(got["eph"], want)
    assert out.TOW == want["SOW"]
