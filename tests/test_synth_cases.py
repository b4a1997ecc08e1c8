"""The generator of synthetic IF records without a GPU: the NumPy restatement (tests/synth_cases.py) reproduces the published
Philox4x32-10 answers, equals csrc/bds_synth_math.h compiled for the host word for word, draws normals with the right moments and
equals synth.make_if on make_if's own symbols; and bds_synth / bds_synth_file refuse bad arguments before any device call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bds_amd
from bds_amd import native, synth

import synth_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


def test_philox_known_answers():
    for ctr, key, want in KNOWN:
        got = " ".join("%08x" % int(w[0]) for w in sc.philox4x32_10(ctr, key))
        assert got == want


def test_header_equals_restatement(tmp_path):
    """csrc/bds_synth_math.h built for the host: words, u1, u2 (bit patterns) and symbols equal the restatement exactly."""
    exe = str(tmp_path / "synth_math_check")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "bds-3-b1c-b2a-sdr-receiver_amd", "csrc"),
                           os.path.join(HERE, "host_models", "synth_math_check.cpp"), "-o", exe])
    rng = np.random.default_rng(1)
    seeds = [0, 3550, 2 ** 64 - 1, 0x0123456789ABCDEF]
    ns = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 33 - 5, 2 ** 53 - 1] + [int(v) for v in rng.integers(0, 2 ** 53, 200)]
    periods = [-2 ** 40, -2, -1, 0, 1, 2 ** 31 - 1, 2 ** 32 - 1, 2 ** 32] + [int(v) for v in rng.integers(-5000, 5000, 100)]
    lines = [f"N {s} {n}" for s in seeds for n in ns] + [f"S {s} {p} {prn} {c}" for s in seeds for p in periods for prn in (1, 19, 63) for c in (0, 1)]
    out = subprocess.check_output([exe], input="\n".join(lines).encode(), timeout=60).decode().split("\n")
    assert [l[2:] for l in out[:3]] == [k[2] for k in KNOWN]
    out = out[3:]
    i = 0
    for s in seeds:
        w = sc.noise_words(s, np.array(ns, dtype=np.int64))
        u1, u2 = sc.noise_uniforms(s, np.array(ns, dtype=np.int64))
        assert (u1 > 0).all() and (u1 < 1).all() and (u2 >= 0).all() and (u2 < 1).all()
        for j in range(len(ns)):
            want = "N %08x %08x %08x %08x %016x %016x" % (*(int(x[j]) for x in w), int(u1[j:j + 1].view(np.uint64)[0]), int(u2[j:j + 1].view(np.uint64)[0]))
            assert out[i] == want, (s, ns[j])
            i += 1
    for s in seeds:
        for p in periods:
            for prn in (1, 19, 63):
                for c in (0, 1):
                    assert out[i] == "S %d" % int(sc.symbols(s, np.array([p]), prn, c)[0]), (s, p, prn, c)
                    i += 1
    assert i == len(lines)


def test_normal_moments():
    """2^20 restated normals (both components): |mean| < 5 / sqrt(n), |var - 1| < 5 sqrt(2 / n), |kurtosis - 3| < 5 sqrt(24 / n)."""
    n = 1 << 20
    for g in sc.noise_normals(3550, np.arange(n, dtype=np.int64)):
        m, v = g.mean(), g.var()
        k = ((g - m) ** 4).mean() / v ** 2
        print("mean %.3e var-1 %.3e kurt-3 %.3e" % (m, v - 1, k - 3))
        assert abs(m) < 5 / np.sqrt(n)
        assert abs(v - 1) < 5 * np.sqrt(2 / n)
        assert abs(k - 3) < 5 * np.sqrt(24 / n)
    a, b = sc.noise_normals(3550, np.arange(n, dtype=np.int64))
    assert abs(np.mean(a * b)) < 5 / np.sqrt(n)  # the two components are uncorrelated
    assert abs(np.mean(a[1:] * a[:-1])) < 5 / np.sqrt(n)  # and so are neighbouring samples


def b1c_case():
    s = bds_amd.init_settings_b1c(samplingFreq=30.69e6, IF=7.5e6)
    return s, [synth.Sat(3, 1250.0, 100.0, 0.7, 47.0), synth.Sat(27, -4321.5, 20000.25, 2.9, 44.0)]


def b2a_case():
    s = bds_amd.init_settings_b2a()
    return s, [synth.Sat(19, 310.0, 36768.75, 1.1, 47.0), synth.Sat(20, -200.0, 70556.25, 0.3, 45.0)]


@pytest.mark.parametrize("case,kw", [(b1c_case, {}), (b1c_case, {"code_doppler": False}), (b1c_case, {"pilot61_secondary": True}), (b2a_case, {})])
def test_restatement_equals_make_if(case, kw):
    """The restatement, given make_if's own symbol draws, against make_if(clean=True).  Bound 8 eps sum(amp) 1.3: the two are the
    same NumPy operations on the same indices, so only the last bits of the products and of sin / cos can differ (a flipped chip
    or symbol would show as 2 amp)."""
    s, sats = case()
    n, seed = 200000, 77
    ref = synth.make_if(s, sats, n, seed=seed, clean=True, **kw)
    got = sc.clean_record(s, sats, 0, n, symbol_table=sc.make_if_symbols(s, sats, n, seed), **kw)
    bound = 8 * np.finfo(np.float64).eps * sc.amp_sum(s, sats) * 1.3
    err = np.abs(got - ref).max()
    print("max |restatement - make_if| = %.3e (bound %.3e)" % (err, bound))
    assert err <= bound


def _call(fmt=1, n_sat=1, prn=19, first=0, n=64, out_bytes=None, size=None, s=None, path=None):
    lib = native.lib()
    cs = native.pack_settings(s or bds_amd.init_settings_b2a())
    arr, o, _ = native.pack_synth([synth.Sat(prn, 100.0, 5.0, 0.1)] * n_sat, fmt, iq_sign=1 if fmt >= 2 else 0)
    if size is not None:
        o.size = size
    if path is not None:
        return lib.bds_synth_file(None, C.byref(cs), n_sat, arr, C.byref(o), first, n, path, 0)
    buf = np.zeros(4096, dtype=np.uint8)
    return lib.bds_synth(None, C.byref(cs), n_sat, arr, C.byref(o), first, n, buf.ctypes.data_as(C.c_void_p),
                         buf.nbytes if out_bytes is None else out_bytes)


def test_argument_checks_come_before_any_device_call(tmp_path):
    """Every argument error is BDS_ERR_ARG with a message, raised with no context at all (so no device call came before it)."""
    err = lambda: native.lib().bds_last_error(None).decode()
    assert _call(size=8) == -1 and "opts.size" in err()
    assert _call(fmt=4) == -1 and "opts.format" in err()
    assert _call(fmt=-1) == -1 and "opts.format" in err()
    assert _call(prn=0) == -1 and "PRN 0" in err()
    assert _call(prn=64) == -1 and "PRN 64" in err()
    assert _call(n_sat=64) == -1 and "n_sat" in err()
    assert _call(fmt=3, first=1, n=64) == -1 and "even" in err()
    assert _call(fmt=3, first=0, n=63) == -1 and "even" in err()
    assert _call(fmt=1, n=64, out_bytes=63) == -1 and "out holds 63 bytes" in err()
    assert _call(fmt=2, n=64, out_bytes=127) == -1 and "take 128" in err()
    assert _call(fmt=0, n=64, out_bytes=511) == -1 and "take 512" in err()
    assert _call(fmt=3, n=64, out_bytes=31) == -1 and "take 32" in err()
    assert _call(first=-1) == -1 and "outside" in err()
    assert _call(s=bds_amd.init_settings_b2a(codeLength=1023)) == -1 and "codeLength" in err()
    p = str(tmp_path / "never_written.bin").encode()
    assert _call(fmt=3, n=63, path=p) == -1 and "even" in err() and not os.path.exists(p)
    # valid arguments get as far as the missing context
    assert _call() == -1 and "ctx is NULL" in err()
    assert _call(fmt=3, first=2, n=64, out_bytes=32) == -1 and "ctx is NULL" in err()
    assert _call(path=p) == -1 and "ctx is NULL" in err() and not os.path.exists(p)
    with pytest.raises(ValueError, match="shape"):
        native.pack_synth([synth.Sat(19, 0.0, 0.0, 0.0)], 1, symbols=np.ones((2, 2, 4), dtype=np.int8))
    with pytest.raises(ValueError, match="packed"):
        synth._device_format(0, False, True)
    with pytest.raises(ValueError, match="clean"):
        synth._device_format(1, True, False)
