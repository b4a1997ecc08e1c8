"""Orbit-driven synthetic IF records without a GPU: bds_synth_trajectory against the physical model solved directly in extended
precision (1 mm of range, for code and carrier), the per-sample arithmetic of csrc/bds_synth_math.h built for the host against
the NumPy restatement bit for bit -- which each altered restatement misses -- and the error exits of bds_synth_trajectory."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bds_amd
from bds_amd import native, synth

import synth_traj_cases as tc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# The bound is set by the purpose, not measured: the README claims millimetres for the fix and the generator must not limit it.
RANGE_BOUND_M = 1e-3


def _settings(signal):
    if signal == "B1C":
        return bds_amd.init_settings_b1c(samplingFreq=12.5e6, IF=3.5e6)
    return bds_amd.init_settings_b2a(samplingFreq=25e6, IF=6.5e6)


@pytest.mark.parametrize("signal", ["B1C", "B2A"])
@pytest.mark.parametrize("seg_log2", [17, 24])
def test_trajectory_against_the_model_solved_directly(signal, seg_log2):
    """40 s, 5 satellites: 10 000 random samples and both sides of every 50th joint, code and carrier within 1 mm of range --
    1e-3 codeFreqBasis / c chips and 1e-3 carrFreqBasis / c cycles.  (float64 alone stays far inside: satpos rounds at ~7e-9 m,
    a cubic over 1.3 s of a MEO range leaves far below a micrometre; profiles/synth_traj_errors.txt has the values measured.)"""
    s = _settings(signal)
    scn = tc.sky_scenario(signal)
    t0 = -0.39 + 1.234e-4
    n_samples = int(40 * s.samplingFreq)
    traj = synth.trajectory(s, scn.ephs, scn.rx, n_samples, scn.tow, t0, seg_log2=seg_log2)
    L = 1 << seg_log2
    assert traj.segs.shape == (5, -(-(n_samples + 32) // L)) and list(traj.prns) == list(scn.prns)
    # the large parts stay out of the polynomials
    assert (traj.segs["code"][..., 0] >= 0).all() and (traj.segs["code"][..., 0] < tc.NCODE).all()
    assert (traj.segs["carr"][..., 0] >= 0).all() and (traj.segs["carr"][..., 0] < 1).all() and (traj.segs["code"][..., 1] > 0).all()
    rng = np.random.default_rng(17)
    joints = np.arange(1, traj.segs.shape[1], 50, dtype=np.int64) * L
    joints = joints[joints < n_samples]
    n = np.concatenate([rng.integers(0, n_samples, 10000), joints - 1, joints, [0, n_samples - 1]])
    code_m, carr_m = tc.phase_errors(s, scn, traj, t0, n)
    print("%s seg_log2 %d: worst |trajectory - truth|: code %.3e m, carrier %.3e m (bound %.0e m)" % (signal, seg_log2, code_m, carr_m, RANGE_BOUND_M))
    assert code_m <= RANGE_BOUND_M and carr_m <= RANGE_BOUND_M
    # neighbours meet at the joint: the cubic of segment j at u = L against segment j + 1 at u = 0, as range
    for k in range(5):
        g = traj.segs[k]
        end_c = ((g["code"][:-1, 3] * L + g["code"][:-1, 2]) * L + g["code"][:-1, 1]) * L + g["code"][:-1, 0] + (g["period0"][:-1] - g["period0"][1:]) * float(tc.NCODE)
        assert np.abs(end_c - g["code"][1:, 0]).max() * tc.C_LIGHT / s.codeFreqBasis <= RANGE_BOUND_M


def _cases():
    """(n, first, seg_log2, segment row) cases for the arithmetic: u = 0, 1, 2^seg_log2 - 1 of several segments, c just below and
    just above a period boundary, negative x, negative period0, a trajectory whose first is not 0 (and one negative)."""
    rng = np.random.default_rng(3)
    out = []
    for first, seg_log2 in ((0, 10), (744, 10), (-5000, 13), (123456789, 26)):
        L = 1 << seg_log2
        segs = np.zeros(4, dtype=native.SYNTH_SEG_DTYPE)
        for j in range(4):
            segs[j]["period0"] = int(rng.integers(-50, 50)) - (40 if j == 1 else 0)
            segs[j]["code"] = [rng.uniform(0, tc.NCODE), rng.uniform(0.01, 0.4), rng.uniform(-1, 1) * 1e-11, rng.uniform(-1, 1) * 1e-18]
            segs[j]["carr"] = [rng.uniform(0, 1), rng.uniform(-0.4, 0.4), rng.uniform(-1, 1) * 1e-9, rng.uniform(-1, 1) * 1e-16]
        segs[2]["carr"][1] = -0.31  # x < 0 from u = 4 on
        # segment 3: c crosses ncode between u = 6 and u = 7, and sits within an ulp or two of it at u = 9
        segs[3]["code"] = [tc.NCODE - 6.5 * 0.25, 0.25, 0.0, 0.0]
        ns = [first + j * L + u for j in range(4) for u in (0, 1, 2, 5, 6, 7, 8, L // 2, L - 2, L - 1)] + [int(v) for v in first + rng.integers(0, 4 * L, 200)]
        out.append((np.array(ns, dtype=np.int64), first, seg_log2, segs))
    # c exactly at, one ulp below and one ulp above the period boundary at u = 0
    segs = np.zeros(3, dtype=native.SYNTH_SEG_DTYPE)
    for j, c0 in enumerate((float(tc.NCODE), np.nextafter(float(tc.NCODE), 0.0), np.nextafter(float(tc.NCODE), 1e9))):
        segs[j]["period0"], segs[j]["code"], segs[j]["carr"] = -7, [c0, 0.3, 0, 0], [0.999999, -1e-3, 0, 0]
    out.append((np.array([0, 1, 1024, 1025, 2048, 2049, 3071], dtype=np.int64), 0, 10, segs))
    return out


@pytest.fixture(scope="module")
def header_output(tmp_path_factory):
    """csrc/bds_synth_math.h built for the host with g++ and run once on every case: per case the (j, u, cph bits, period, th bits)."""
    exe = str(tmp_path_factory.mktemp("traj") / "synth_traj_check")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "bds-3-b1c-b2a-sdr-receiver_amd", "csrc"),
                           os.path.join(HERE, "host_models", "synth_traj_check.cpp"), "-o", exe])
    hx = lambda v: "%016x" % int(np.float64(v).view(np.uint64))  # noqa: E731
    results = []
    for ns, first, seg_log2, segs in _cases():
        phase = 0.7
        j = (ns - first) >> seg_log2  # the header is given the segment of the RIGHT index; it computes j and u itself
        lines = ["%d %d %d %d %s %s" % (n, first, seg_log2, g["period0"], " ".join(hx(v) for v in list(g["code"]) + list(g["carr"])), hx(phase))
                 for n, g in zip(ns, segs[j])]
        out = subprocess.check_output([exe], input="\n".join(lines).encode(), timeout=60).decode().split()
        a = np.array(out).reshape(len(ns), 5)
        results.append((a[:, 0].astype(np.int64), a[:, 1].astype(np.int64), np.array([int(v, 16) for v in a[:, 2]], dtype=np.uint64),
                        a[:, 3].astype(np.int64), np.array([int(v, 16) for v in a[:, 4]], dtype=np.uint64)))
    return results


def _mismatches(header_output, model):
    """Number of cases at which the restatement under `model` differs from the header in any of j, u, cph, period, th (bit patterns)."""
    bad = 0
    for (ns, first, seg_log2, segs), want in zip(_cases(), header_output):
        j, u, cph, period, th = tc.sample_arith(segs, first, seg_log2, ns, 0.7, model)
        got = (j, u, cph.view(np.uint64), period, th.view(np.uint64))
        bad += int(np.any([g != w for g, w in zip(got, want)], axis=0).sum())
    return bad


def test_header_arithmetic_equals_the_restatement_bit_for_bit(header_output):
    cases = _cases()
    # the cases are what they claim
    ns, first, seg_log2, segs = cases[1]
    j, u, cph, period, th = tc.sample_arith(segs, first, seg_log2, ns)
    L = 1 << seg_log2
    assert first != 0 and {0, 1, L - 1} <= set(u.tolist()) and set(j.tolist()) == {0, 1, 2, 3}
    x = tc._poly(segs[j]["carr"], u.astype(np.float64), tc.RIGHT)
    assert (x < 0).any() and (x > 0).any() and (segs["period0"] < 0).any()
    at = lambda uu: period[(j == 3) & (u == uu)][0]  # noqa: E731
    assert at(7) == at(6) + 1 == segs[3]["period0"] + 1  # the period rolls over between u = 6 and u = 7
    ns, first, seg_log2, segs = cases[-1]
    _, _, cph, period, _ = tc.sample_arith(segs, first, seg_log2, ns)
    assert list(period[[0, 2, 4]]) == [-6, -7, -6] and cph[0] == 0 and cph[2] == np.nextafter(float(tc.NCODE), 0.0)
    assert _mismatches(header_output, tc.RIGHT) == 0


@pytest.mark.parametrize("name", sorted(tc.ALTERED))
def test_an_altered_restatement_is_caught(header_output, name):
    """One change each -- Horner order, floor for trunc, the segment index off by one at a joint, period0 ignored -- fails the
    comparison that the right restatement passes."""
    n = _mismatches(header_output, tc.ALTERED[name])
    print(name, "differs at", n, "cases")
    assert n > 0


def test_trajectory_methods_are_the_restatement():
    """Trajectory.code_phase / carrier_phase are sample_arith's values for every row at once."""
    s = _settings("B1C")
    t = tc.hand_made(s)
    traj = synth.Trajectory(t.segs, t.first, t.seg_log2, np.array([19, 27, 19], dtype=np.int32))
    n = np.arange(1000, 5120, dtype=np.int64)
    cph, period = traj.code_phase(n)
    x = traj.carrier_phase(n)
    for k in range(3):
        _, _, c, p, th = tc.sample_arith(t.segs[k], t.first, t.seg_log2, n, 0.0)
        assert np.array_equal(c, cph[k]) and np.array_equal(p, period[k])
        assert np.array_equal(th, 2 * np.pi * (x[k] - np.trunc(x[k])) + 0.0)
    # the hand-made rows do what the GPU tests need: a roll-over 1, 2 and 3 samples from a joint, a negative period0, negative x
    roll = [int(n[np.nonzero(np.diff(period[k]) == 1)[0][0] + 1]) - t.first for k in range(3)]
    assert roll == [2047, 2049, 3071] and (t.segs["period0"] < 0).any() and (x[2] < 0).mean() > 0.99
    with pytest.raises(ValueError, match="outside the trajectory"):
        traj.code_phase(np.array([t.first - 1]))


@pytest.mark.parametrize("signal", ["B1C", "B2A"])
def test_tiny_records_exclude_at_most_one_sample_in_4096(signal):
    """The records of the GPU bit-equality tests, restated: for the chosen seed at most 1 value in 4096 lies within 1e-9 of a
    rounding boundary of the quantiser (the only places where tests/test_synth_traj_gpu.py lets formats 1 and 2 differ), and the
    restated clean record is a signal (not zeros, not clipped)."""
    import synth_cases as sc

    s = _settings(signal)
    t = tc.hand_made(s)
    sats = tc.tiny_sats()
    traj = synth.Trajectory(t.segs, t.first, t.seg_log2, np.array([x.prn for x in sats], dtype=np.int32))
    z = tc.clean_record(s, sats, traj, tc.TINY_FIRST, tc.TINY_N, seed=tc.TINY_SEED)
    assert 0.5 * sc.amp_sum(s, sats[:1]) < np.abs(z.real).max() <= sc.amp_sum(s, sats) * 1.5  # |s_I + j s_Q| <= sqrt(2) (B2a), 1.3 (B1C)
    for iq_sign in (0, 1, -1):
        v = tc.record_values(z, tc.TINY_FIRST, seed=tc.TINY_SEED, iq_sign=iq_sign)
        n_ex = int(sc.near_boundary(v).sum())
        print(signal, "iq_sign", iq_sign, ":", n_ex, "of", v.size, "values excluded")
        assert n_ex <= v.size // 4096 and np.abs(v).max() < 127


def _trajectory_rc(s=None, ephs=None, rx=None, seg_log2=17, n_seg=2, out=True, null=None):
    scn = tc.sky_scenario("B1C")
    s = s or _settings("B1C")
    cs = native.pack_settings(s)
    arr = native.eph_array(scn.ephs[:2] if ephs is None else ephs)
    r = np.ascontiguousarray(scn.rx if rx is None else rx, dtype=np.float64)
    buf = np.zeros((2, max(n_seg, 1)), dtype=native.SYNTH_SEG_DTYPE)
    args = [C.byref(cs), 2, arr, r.ctypes.data_as(native._DP), float(scn.tow), -0.39, 0, n_seg, seg_log2, buf.ctypes.data_as(C.POINTER(native.SynthSeg))]
    if null is not None:
        args[null] = None
    return native.lib().bds_synth_trajectory(*args)


def test_trajectory_refuses_bad_arguments():
    """Every argument error of bds_synth_trajectory is BDS_ERR_ARG with a message; there is no context and no device in this entry."""
    err = lambda: native.lib().bds_last_error(None).decode()  # noqa: E731
    scn = tc.sky_scenario("B1C")
    assert _trajectory_rc() == 0
    for null in (0, 2, 3, 9):
        assert _trajectory_rc(null=null) == -1 and "is NULL" in err()
    assert _trajectory_rc(seg_log2=9) == -1 and "seg_log2 = 9" in err()
    assert _trajectory_rc(seg_log2=27) == -1 and "seg_log2 = 27" in err()
    assert _trajectory_rc(n_seg=0) == -1 and "n_seg = 0" in err()
    assert _trajectory_rc(ephs=[scn.ephs[0], dict(scn.ephs[1], flag=0)]) == -1 and "eph[1] is not ready" in err()
    assert _trajectory_rc(ephs=[dict(scn.ephs[0], SatType=0), scn.ephs[1]]) == -1 and "eph[0]: unknown SatType 0" in err()
    assert _trajectory_rc(rx=[np.nan, 0.0, 0.0]) == -1 and "not finite" in err()
    assert _trajectory_rc(s=_settings("B1C").copy(codeFreqBasis=0.0)) == -1 and "code rate must be positive" in err()
    assert _trajectory_rc(s=_settings("B1C").copy(codeFreqBasis=-1.023e6)) == -1 and "code rate must be positive" in err()
    with pytest.raises(native.BdsError, match="seg_log2 = 5"):
        synth.trajectory(_settings("B1C"), scn.ephs, scn.rx, 1000, scn.tow, -0.39, seg_log2=5)


def _traj_call(entry="bds_synth_traj", fmt=1, first=1000, n=64, size=None, doppler=0.0, seg_edit=None, traj_null=False):
    s = _settings("B1C")
    t = tc.hand_made(s)
    segs = t.segs.copy()
    if seg_edit:
        seg_edit(segs)
    cs = native.pack_settings(s)
    sats = [synth.Sat(19, doppler, 0.0, 0.1), synth.Sat(27, 0.0, 0.0, 0.2), synth.Sat(19, 0.0, 0.0, 0.3)]
    arr, o, _ = native.pack_synth(sats, fmt, iq_sign=1 if fmt >= 2 else 0)
    tr, keep = native.pack_traj(segs, t.first, t.seg_log2, 3)
    if size is not None:
        tr.size = size
    buf = np.zeros(8192, dtype=np.uint8)
    return getattr(native.lib(), entry)(None, C.byref(cs), 3, arr, C.byref(o), None if traj_null else C.byref(tr), first, n,
                                        buf.ctypes.data_as(C.c_void_p), buf.nbytes)


@pytest.mark.parametrize("entry", ["bds_synth_traj", "bds_synth_traj_dev"])
def test_generator_checks_come_before_any_device_call(entry):
    """Each error of the trajectory path is BDS_ERR_ARG with a message, raised with no context at all (so no device call came
    before it); valid arguments get as far as the missing context."""
    err = lambda: native.lib().bds_last_error(None).decode()  # noqa: E731
    assert _traj_call(entry) == -1 and "ctx is NULL" in err()
    assert _traj_call(entry, first=743) == -1 and "outside the trajectory" in err()
    assert _traj_call(entry, first=744 + 6 * 1024 - 64, n=64) == -1 and "ctx is NULL" in err()  # the last 64 samples: 4 whole units
    assert _traj_call(entry, first=744 + 6 * 1024 - 64, n=65) == -1 and "outside the trajectory" in err()
    assert _traj_call(entry, first=744 + 6 * 1024 - 63, n=49) == -1 and "outside the trajectory" in err()  # the unit made whole runs past the end
    assert _traj_call(entry, size=24) == -1 and "traj.size = 24" in err()
    assert _traj_call(entry, traj_null=True) == -1 and "traj is NULL" in err()

    def nan(segs):
        segs[1, 3]["carr"][2] = np.nan

    def inf(segs):
        segs[2, 0]["code"][0] = np.inf

    def slow(segs):
        segs[0, 5]["code"][1] = 0.0

    def back(segs):
        segs[1, 2]["code"][1] = -0.08

    assert _traj_call(entry, seg_edit=nan) == -1 and "satellite 2, segment 3: a coefficient is not finite" in err()
    assert _traj_call(entry, seg_edit=inf) == -1 and "satellite 3, segment 0: a coefficient is not finite" in err()
    assert _traj_call(entry, seg_edit=slow) == -1 and "satellite 1, segment 5: code[1] = 0" in err()
    assert _traj_call(entry, seg_edit=back) == -1 and "code rate must be positive" in err()
    assert _traj_call(entry, doppler=100.0) == -1 and "doppler = 100" in err()
    assert _traj_call(entry, fmt=3, first=1001) == -1 and "even" in err()
    assert _traj_call(entry, fmt=4) == -1 and "opts.format" in err()
    s = _settings("B1C")
    t = tc.hand_made(s)
    traj = synth.Trajectory(t.segs, t.first, t.seg_log2, np.array([19, 27, 19]))
    with pytest.raises(ValueError, match="doppler = 0.0, delay = 5.0"):
        synth.make_if_device(s, [synth.Sat(19, 0.0, 5.0, 0.1)] * 3, 64, first_sample=1000, trajectory=traj)
