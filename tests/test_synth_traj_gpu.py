"""bds_synth_traj / bds_synth_traj_dev on the device: bit equality with the NumPy restatement (tests/synth_traj_cases.py) on tiny
records whose hand-made trajectories put a code-period roll-over and a symbol change within three samples of a joint; records made
in pieces; the error exits; and one run that ties the whole chain together at the signal level -- a receiver position and
ephemerides in, a 37 s B1C record, tracking, navigation decoding and the position fix out.

The tiny records: 3 satellites, PRN 19 twice, segments of 1024 samples from sample 744 on, samples 1000 .. 5119 (four joints
inside, first_sample no multiple of 32).  The restated records are computed once per module."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import bds_amd
from bds_amd import native, synth

import pvt_cases as pc
import synth_cases as sc
import synth_traj_cases as tc
from packed_cases import pack_iq, quantise

pytestmark = pytest.mark.gpu

SEED, FIRST, N = tc.TINY_SEED, tc.TINY_FIRST, tc.TINY_N
SATS = tc.tiny_sats()


def _settings(name):
    return bds_amd.init_settings_b1c(samplingFreq=12.5e6, IF=3.5e6) if name == "b1c" else bds_amd.init_settings_b2a(samplingFreq=25e6, IF=6.5e6)


def _traj(s):
    t = tc.hand_made(s)
    return synth.Trajectory(t.segs, t.first, t.seg_log2, np.array([x.prn for x in SATS], dtype=np.int32))


@pytest.fixture(scope="module")
def refs():
    """Per signal: settings, trajectory, the restated clean complex record of samples FIRST .. FIRST + N, the noise."""
    out = {}
    for name in ("b1c", "b2a"):
        s = _settings(name)
        traj = _traj(s)
        z = tc.clean_record(s, SATS, traj, FIRST, N, seed=SEED)
        # the cases are what they claim: roll-overs 1, 2 and 3 samples from a joint, a symbol change with one of them
        _, period = traj.code_phase(np.arange(FIRST, FIRST + N, dtype=np.int64))
        roll = [int(np.nonzero(np.diff(period[k]) == 1)[0][0]) + 1 + FIRST - traj.first for k in range(3)]
        assert roll == [2047, 2049, 3071] and traj.first != 0 and FIRST % 32 != 0
        changes = [sc.symbols(SEED, np.array([period[k][r - 1 - (FIRST - traj.first)], period[k][r - (FIRST - traj.first)]]), SATS[k].prn, c)
                   for k, r in enumerate(roll) for c in (0, 1)]
        assert any(a != b for a, b in changes)
        out[name] = SimpleNamespace(s=s, traj=traj, z=z)
    return out


@pytest.mark.parametrize("name", ["b1c", "b2a"])
def test_format_0_equals_the_restatement_bit_for_bit(ctx, refs, name):
    r = refs[name]
    got = synth.make_if_device(r.s, SATS, N, seed=SEED, first_sample=FIRST, clean=True, trajectory=r.traj)
    assert got.dtype == np.float64 and got.shape == (N,)
    bad = np.nonzero(got.view(np.uint64) != r.z.real.copy().view(np.uint64))[0]
    print("%s: %d of %d samples differ from the restatement; worst %.3e" % (name, bad.size, N, np.abs(got - r.z.real).max()))
    assert bad.size == 0, (bad[:8] + FIRST, got[bad[:8]], r.z.real[bad[:8]])
    assert np.abs(got).max() > 0.5 * sc.amp_sum(r.s, SATS[:1])


@pytest.mark.parametrize("name", ["b1c", "b2a"])
@pytest.mark.parametrize("iq_sign", [0, 1, -1])
def test_int8_records_equal_the_restatement(ctx, refs, name, iq_sign):
    """Formats 1 and 2: equal except where |v - rint(v)| is within 1e-9 of a half (the device's log, sqrt and cos of the noise differ
    from NumPy's by a few ulp); no more than 1 sample in 4096 is excluded, an excluded one is off by at most 1."""
    r = refs[name]
    v = tc.record_values(r.z, FIRST, seed=SEED, iq_sign=iq_sign)
    ex = sc.near_boundary(v)
    assert ex.sum() <= max(1, v.size // 4096)
    got = synth.make_if_device(r.s, SATS, N, seed=SEED, first_sample=FIRST, iq_sign=iq_sign, trajectory=r.traj)
    assert got.dtype == np.int8 and got.shape == v.shape
    want = sc.quantise8(v)
    np.testing.assert_array_equal(got[~ex], want[~ex])
    assert np.abs(got[ex].astype(np.int16) - want[ex]).max(initial=0) <= 1
    assert got.std() > 15


@pytest.mark.parametrize("name", ["b1c", "b2a"])
def test_packed_record_is_the_quantised_iq_record(ctx, refs, name):
    """Format 3 = the packed form of the format-2 record, at the default threshold and at 5."""
    r = refs[name]
    for thr in (None, 5.0):
        pairs = synth.make_if_device(r.s, SATS, N, seed=SEED, first_sample=FIRST, iq_sign=-1, trajectory=r.traj)
        packed = synth.make_if_device(r.s, SATS, N, seed=SEED, first_sample=FIRST, iq_sign=-1, packed=True, threshold=thr, trajectory=r.traj)
        assert packed.dtype == np.uint8 and packed.size == N // 2
        np.testing.assert_array_equal(packed, pack_iq(quantise(pairs, **({} if thr is None else {"threshold": thr}))))


PIECES = [1, 31, 32, 33, 1500]


def _cuts():
    cuts, i = [0], 0
    while cuts[-1] < N:
        cuts.append(min(N, cuts[-1] + PIECES[i % len(PIECES)]))
        i += 1
    return list(zip(cuts[:-1], cuts[1:]))


@pytest.mark.parametrize("fmt", [0, 1])
def test_pieces_in_any_order_equal_one_call(ctx, refs, fmt):
    """Pieces of 1, 31, 32, 33 and 1500 samples, made last piece first, through bds_synth_traj and through bds_synth_traj_dev into
    a misaligned tensor: the one-call record bit for bit."""
    import torch

    r = refs["b1c"]
    kw = {"clean": True} if fmt == 0 else {}
    whole = synth.make_if_device(r.s, SATS, N, seed=SEED, first_sample=FIRST, trajectory=r.traj, **kw)
    cuts = _cuts()
    assert {b - a for a, b in cuts} >= set(PIECES)
    host = np.zeros_like(whole)
    buf = torch.zeros(N + 1, dtype=torch.float64 if fmt == 0 else torch.int8, device="cuda:0")
    dev = buf[1:]  # 8 bytes (format 0) or 1 byte (format 1) off the allocation's 16-byte alignment
    assert dev.data_ptr() % 16 != 0
    for a, b in reversed(cuts):
        host[a:b] = synth.make_if_device(r.s, SATS, b - a, seed=SEED, first_sample=FIRST + a, trajectory=r.traj, **kw)
        ctx.synth_traj_dev(r.s, SATS, r.traj, FIRST + a, b - a, fmt, dev[a:b], seed=SEED)
    np.testing.assert_array_equal(host.view(np.uint8), whole.view(np.uint8))
    np.testing.assert_array_equal(dev.cpu().numpy().view(np.uint8), whole.view(np.uint8))
    assert buf[0].item() == 0  # nothing outside the record was written
    one = synth.make_if_device(r.s, SATS, N, seed=SEED, first_sample=FIRST, trajectory=r.traj, out="torch", **kw)
    np.testing.assert_array_equal(one.cpu().numpy().view(np.uint8), whole.view(np.uint8))


def test_error_exits_come_with_a_message(ctx, refs):
    r = refs["b1c"]
    mk = lambda **kw: synth.make_if_device(r.s, kw.pop("sats", SATS), kw.pop("n", 64), seed=SEED, **dict(dict(first_sample=FIRST, trajectory=r.traj), **kw))  # noqa: E731
    with pytest.raises(native.BdsError, match="outside the trajectory"):
        mk(first_sample=r.traj.first - 1)
    with pytest.raises(native.BdsError, match="outside the trajectory"):
        mk(first_sample=r.traj.first + 6 * 1024 - 64, n=65)
    assert mk(first_sample=r.traj.first + 6 * 1024 - 64, n=64).size == 64  # the trajectory's last samples
    for edit, msg in (((1, 3, "carr", 2, np.nan), "satellite 2, segment 3: a coefficient is not finite"),
                      ((0, 5, "code", 1, 0.0), "code rate must be positive"), ((2, 1, "code", 1, -0.08), "code rate must be positive")):
        segs = r.traj.segs.copy()
        segs[edit[0], edit[1]][edit[2]][edit[3]] = edit[4]
        with pytest.raises(native.BdsError, match=msg):
            mk(trajectory=synth.Trajectory(segs, r.traj.first, r.traj.seg_log2, r.traj.prns))
    with pytest.raises(ValueError, match="doppler = 250.0"):
        mk(sats=[synth.Sat(19, 250.0, 0.0, 0.7, 47.0)] + SATS[1:])
    with pytest.raises(native.BdsError, match="even"):
        mk(first_sample=FIRST + 1, iq_sign=1, packed=True)
    # the size field and a non-zero doppler at the C entry itself
    cs = native.pack_settings(r.s)
    arr, o, _ = native.pack_synth(SATS, 1)
    t, keep = native.pack_traj(r.traj.segs, r.traj.first, r.traj.seg_log2, 3)
    out = np.zeros(64, dtype=np.int8)
    call = lambda: ctx._lib.bds_synth_traj(ctx._h, C.byref(cs), 3, arr, C.byref(o), C.byref(t), FIRST, 64, out.ctypes.data_as(C.c_void_p), out.nbytes)  # noqa: E731
    assert call() == 0
    t.size = 40
    assert call() == -1 and "traj.size = 40" in ctx._lib.bds_last_error(ctx._h).decode()
    t.size = C.sizeof(native.SynthTraj)
    arr[1].doppler = -3.0
    assert call() == -1 and "satellite 2: doppler = -3" in ctx._lib.bds_last_error(ctx._h).decode()


# ---- position in, position out ---------------------------------------------------------------------------------------------------------
N_EPOCHS = 3700
CN0_DBHZ = 50.0


def _scenario():
    """Five satellites at 50 dB-Hz seen from the scenario's receiver, each with its own B-CNAV1 frame: code period P = 0 is the
    frame's first symbol (element (P + 1) mod n_sym = 1 of the rows), the periods before it read the table's tail."""
    s = bds_amd.init_settings_b1c(samplingFreq=12.5e6, IF=3.5e6, FEBW=10e6, pilotTRKflag=2, CNoInterval=50, useTropCorr=0,
                                  msToProcess=N_EPOCHS * 10, numberOfChannels=5)
    scn = tc.sky_scenario("B1C", seed=23)
    rng = np.random.default_rng(23)
    spc = int(round(s.samplingFreq * s.codeLength / s.codeFreqBasis))
    n_samples = (N_EPOCHS + 3) * spc
    # t0: every frame arrives 0.45 s or later after sample 0, past epoch 41 and the loops' transient
    delay0 = [float(tc.truth_phases(s, e, scn.rx, scn.tow, 0.0, np.array([0]))[2][0]) for e in scn.ephs]
    t0 = min(delay0) - 0.45 + 1.234e-4
    traj = synth.trajectory(s, scn.ephs, scn.rx, n_samples, scn.tow, t0)
    n_sym = N_EPOCHS + 100
    rows = rng.choice(np.array([-1, 1], dtype=np.int8), (5, 2, n_sym))
    period_of = np.arange(n_sym) - 1
    period_of[period_of > N_EPOCHS + 10] -= n_sym  # the tail: the periods before P = 0
    for k, prn in enumerate(scn.prns):
        rows[k, 0, 1:1801] = synth.bcnav1_symbols(scn.msgs[k][0].copy(), fill=rng.integers(0, 2, 864))
        rows[k, 1] = native.gen_code("B1C", "pilot_secondary", int(prn))[period_of % 1800]
    return SimpleNamespace(s=s, scn=scn, t0=t0, traj=traj, rows=rows, n_samples=n_samples, spc=spc)


def test_position_in_position_out_b1c(ctx):
    """The bounds are derived, not tuned.
    Position, per fix: 4 PDOP sigma_rho with PDOP from the solver's own DOP output and the early-minus-late code noise of a
    non-coherent DLL, sigma_rho = (c / codeFreqBasis) sqrt(B_L d / (2 C/N0_p)) sqrt(1 + 2 / ((2 - d) T C/N0_p)): B_L =
    dllNoiseBandwidth = 1 Hz, d = 2 dllCorrelatorSpacing = 0.12 chips (taps at -+0.06), T = 10 ms, C/N0_p = 3/4 of 50 dB-Hz (the pilot
    is 1/11 + 29/44 of B1C's power).  That is the BPSK formula, an upper bound for the sharper BOC peak: 0.262 m.  The factor 4 lets
    none of the fixes fall outside by chance.  The mean error over the fixes is held to the same bound (with the largest PDOP)
    over the square root of the number of fixes spaced 1 / (2 B_L) = 0.5 s apart.
    Carrier frequency: the NCO frequency of an epoch is the loop filter's output, whose proportional branch alone passes the
    discriminator's noise with gain pf1 = 2 wn = 2.4 pllNoiseBandwidth [Hz per cycle]: sigma_f = pf1 sigma_d, sigma_d the noise of
    the wide-band discriminator (atan(Q / I) of data and pilot weighted 1 : 3) = sqrt(s_d^2 + 9 s_p^2) / 4 / (2 pi) cycles with
    s^2 = 1 / (2 T C/N0) of each component: 0.10 Hz.  The mean of carrFreq - truth over the epochs after the transient is held
    below that one-epoch noise, and the fitted slope to the truth's within 2 sigma_f over the span."""
    c = _scenario()
    s, scn, traj = c.s, c.scn, c.traj
    sats = [synth.Sat(int(p), 0.0, 0.0, 0.3 + k, CN0_DBHZ) for k, p in enumerate(scn.prns)]
    rec = synth.make_if_device(s, sats, c.n_samples, seed=77, symbols=c.rows, pilot61_secondary=True, out="torch", trajectory=traj)
    assert rec.numel() == c.n_samples
    # the channels from the trajectory's truth: the first sample of the first whole code period, carrier and code rate there
    cph0, p0 = traj.code_phase(np.array([0]))
    chans, sfs_want = [], []
    for k in range(5):
        guess = int((tc.NCODE - cph0[k, 0]) / traj.segs[k, 0]["code"][1])
        near = np.arange(max(guess - 3, 0), guess + 4, dtype=np.int64)
        start = int(near[np.nonzero(traj.code_phase(near)[1][k] == p0[k, 0] + 1)[0][0]])
        at = np.array([start])
        chans.append(SimpleNamespace(PRN=int(scn.prns[k]), acquiredFreq=float(s.samplingFreq * traj.carrier_rate(at)[k, 0]), codePhase=float(start + 1),
                                     codeFreq=float(s.samplingFreq * traj.segs[k, 0]["code"][1]), status="T"))
        sfs_want.append(-int(p0[k, 0]))  # epoch 1 is period p0 + 1, so period 0 is epoch -p0
    assert min(sfs_want) > 41
    res, _ = bds_amd.tracking(rec, chans, s)
    del rec
    assert all(r.status == "T" and r.completed == N_EPOCHS for r in res)
    dec = bds_amd.nav_decode(res, s)
    assert [d.firstSubFrame for d in dec] == sfs_want and all(d.TOW == scn.tow for d in dec)
    nav, eph = bds_amd.post_navigation(res, s)
    assert nav is not None and (nav.channelStatus == pc.READY).all()
    for k, prn in enumerate(scn.prns):
        for f in (f for f in native.EPH_FIELDS if f != "TOW"):
            want = scn.ephs[k][f]
            got = getattr(eph[int(prn)], f, None)
            assert (got is None or np.isnan(got)) if np.isnan(want) else got == want, (k, f, got, want)
    # -- the fixes
    T, b_l, d = s.intTime, s.dllNoiseBandwidth, 2 * s.dllCorrelatorSpacing
    cn0_p = 0.75 * 10 ** (CN0_DBHZ / 10)
    sigma_rho = (tc.C_LIGHT / s.codeFreqBasis) * np.sqrt(b_l * d / (2 * cn0_p)) * np.sqrt(1 + 2 / ((2 - d) * T * cn0_p))
    err_xyz = np.stack([nav.X - scn.rx[0], nav.Y - scn.rx[1], nav.Z - scn.rx[2]])
    err = np.sqrt((err_xyz ** 2).sum(axis=0))
    pdop = nav.DOP[1]
    n_fix = err.size
    span_s = (nav.currMeasSample[-1] - nav.currMeasSample[0]) / s.samplingFreq
    n_indep = int(span_s * 2 * b_l) + 1
    mean_err = float(np.sqrt((err_xyz.mean(axis=1) ** 2).sum()))
    mean_bound = 4 * pdop.max() * sigma_rho / np.sqrt(n_indep)
    print("position: %d fixes over %.1f s (%d spaced 0.5 s apart), PDOP %.3f .. %.3f, sigma_rho %.4f m; worst error %.4f m (bound %.4f m at its "
          "fix), error of the mean fix %.4f m (bound %.4f m)" % (n_fix, span_s, n_indep, pdop.min(), pdop.max(), sigma_rho, err.max(),
                                                                 4 * pdop[err.argmax()] * sigma_rho, mean_err, mean_bound))
    # -- the carrier
    wn = 1.2 * s.pllNoiseBandwidth
    sd2, sp2 = 1 / (2 * T * 0.25 * 10 ** (CN0_DBHZ / 10)), 1 / (2 * T * cn0_p)
    sigma_f = 2 * wn * np.sqrt(sd2 + 9 * sp2) / 4 / (2 * np.pi)
    after = slice(100, N_EPOCHS)
    worst_mean = worst_slope = 0.0
    for k, r in enumerate(res):
        at = np.asarray(r.absoluteSample, dtype=np.float64)[after].astype(np.int64)
        truth = s.samplingFreq * traj.carrier_rate(at)[k]
        got = np.asarray(r.carrFreq, dtype=np.float64)[after]
        t = (at - at[0]) / s.samplingFreq
        slope_got, slope_true = np.polyfit(t, got, 1)[0], np.polyfit(t, truth, 1)[0]
        print("PRN %d: carrFreq - truth mean %+.4f Hz (sigma_f %.4f Hz), slope %+.5f Hz/s against %+.5f Hz/s" % (r.PRN, (got - truth).mean(), sigma_f,
                                                                                                              slope_got, slope_true))
        # a slope a constant-Doppler record cannot produce: the truth moves by more than 4 sigma_f over the span
        assert abs(slope_true) * t[-1] > 4 * sigma_f
        worst_mean = max(worst_mean, abs(float((got - truth).mean())))
        worst_slope = max(worst_slope, abs(slope_got - slope_true) * t[-1])
    assert worst_mean < sigma_f and worst_slope <= 2 * sigma_f
    assert n_fix >= 70 and (err <= 4 * pdop * sigma_rho).all()
    assert mean_err <= mean_bound
