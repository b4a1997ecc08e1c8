"""The pulse blanker without a GPU: the fast model equals the definition, pieces with their context reproduce the whole (and
pieces with one sample too little do not), blank_threshold's estimator on clean and jammed histograms, the interference
generator, the argument refusals of the three entries before any device call, and the jammed scene on the float64 oracle."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import bds_amd
from bds_amd import native, synth
from oracle import acquisition as oacq

import blank_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def scene():
    return bc.dme_scenario()


def test_fast_model_equals_the_definition():
    for name, fmt, rec, tsq, pre, post in bc.small_cases():
        for lead, tail, ds in ((0, 0, 0), (0, 0, 7), (11, 13, 50)):
            a, ra = bc.model(rec, fmt, tsq, pre, post, lead, tail, ds, blanked=bc.blanked_brute)
            b, rb = bc.model(rec, fmt, tsq, pre, post, lead, tail, ds, blanked=bc.blanked_fast)
            np.testing.assert_array_equal(a, b, err_msg=f"{name} {fmt}")
            assert {k: v for k, v in ra.items() if k != "duty"} == {k: v for k, v in rb.items() if k != "duty"}
            if ds:
                np.testing.assert_array_equal(ra["duty"], rb["duty"])
                assert ra["duty"].sum() == ra["n_blanked"] and ra["duty"].size == -(-ra["n_samples"] // ds)
    runs = {name: bc.model(rec, fmt, tsq, pre, post)[1]["n_runs"] for name, fmt, rec, tsq, pre, post in bc.small_cases() if fmt == "s8c"}
    assert (runs["none"], runs["all"], runs["one_run"], runs["two_runs"], runs["wide"]) == (0, 1, 1, 2, 1)


@pytest.mark.parametrize("fmt", list(bc.FORMATS))
def test_pieces_with_context_reproduce_the_whole(fmt):
    n, piece, pre, post = 1000, 100, 7, 12
    # hits exactly `post` in front of a seam and `pre` behind one: the first and last sample of a piece hang on the context's last sample
    rec = bc.with_hits(fmt, n, [300 - post, 500 + pre - 1, 17, 640, 641, 999], seed=1)
    whole, rep = bc.model(rec, fmt, 2500, pre, post)
    got, tot = bc.pieces(rec, fmt, 2500, pre, post, piece, post, pre)
    np.testing.assert_array_equal(got, whole)
    assert tot[:2] == (rep["n_flagged"], rep["n_blanked"])
    got, tot = bc.pieces(rec, fmt, 2500, pre, post, piece, post + 1, pre)  # one more sample in front: the run count adds up as well
    np.testing.assert_array_equal(got, whole)
    assert tot == (rep["n_flagged"], rep["n_blanked"], rep["n_runs"])
    assert not np.array_equal(bc.pieces(rec, fmt, 2500, pre, post, piece, post - 1, pre)[0], whole)
    assert not np.array_equal(bc.pieces(rec, fmt, 2500, pre, post, piece, post, pre - 1)[0], whole)


def _probe_like(rec):
    h = np.bincount(rec.astype(np.int64) + 128, minlength=257)
    return SimpleNamespace(hist_i=h, hist_q=None, bins=np.arange(-128, 129), min=int(rec.min()), max=int(rec.max()))


def test_blank_threshold_on_clean_and_jammed_histograms(scene):
    """true sigma = 20; measured: 20.2 clean, 21.4 at 20 000 pairs/s, 22.7 at 40 000 (plain 1.4826 MAD gives 26.7 at 20 000)"""
    s = scene.settings
    p2 = synth.dme_pulses(s, scene.clean.size, pairs_per_s=40000, peak=400, f_offset=1e6, seed=7)
    j2 = np.clip(np.rint(scene.clean.astype(np.float64) + p2), -127, 127).astype(np.int8)
    clean, j20, j40 = (bds_amd.blank_threshold(_probe_like(r), k=1.0) for r in (scene.clean, scene.jammed, j2))
    assert abs(clean - 20.0) <= 0.02 * 20.0
    assert abs(j20 - 20.0) <= 0.10 * 20.0
    assert 5.0 * j20 < 127 and clean < j20 < j40 < 25.0
    assert bds_amd.blank_threshold(_probe_like(scene.jammed)) == 5.0 * j20
    iq = SimpleNamespace(hist_i=_probe_like(scene.clean).hist_i, hist_q=_probe_like(scene.jammed).hist_i, bins=np.arange(-128, 129), min=(-127, -127), max=(127, 127))
    assert bds_amd.blank_threshold(iq, k=1.0) == pytest.approx(np.sqrt(0.5 * (clean ** 2 + j20 ** 2)), rel=1e-12)
    with pytest.raises(ValueError, match="int16"):
        bds_amd.blank_threshold(_probe_like(scene.clean), settings=s.copy(dataType="int16"))


def test_dme_pulses_is_deterministic_in_its_seed(scene):
    s = scene.settings
    a = synth.dme_pulses(s, 50000, 20000, 400, 1e6, seed=7)
    b = synth.dme_pulses(s, 50000, 20000, 400, 1e6, seed=7)
    c = synth.dme_pulses(s, 50000, 20000, 400, 1e6, seed=8)
    assert a.dtype == np.float64 and np.array_equal(a, b) and not np.array_equal(a, c)
    z = synth.dme_pulses(s, 50000, 20000, 400, 1e6, seed=7, iq_sign=1)
    zc = synth.dme_pulses(s, 50000, 20000, 400, 1e6, seed=7, iq_sign=-1)
    assert z.dtype == np.complex128 and np.allclose(z.real, a, atol=1e-9) and np.array_equal(zc, np.conj(z))
    assert 390 < np.abs(z).max() < 2 * 400 + 1 and np.count_nonzero(a) < a.size
    assert not synth.dme_pulses(s, 50000, 0, 400, 1e6, seed=7).any()


def _call(entry="bds_blank", fmt="s8", n_bytes=64, pre=1, post=1, lead=0, tail=0, ds=0, cap=None, out_shift=None, s=None, piece=0, paths=None):
    lib = native.lib()
    cs = native.pack_settings(s or bc.settings_of(fmt))
    o, rep, _ = native.pack_blank(2500, pre, post, lead, tail, ds)
    duty = np.zeros(64, dtype=np.int32)
    if cap is not None:
        rep.duty, rep.duty_cap = duty.ctypes.data_as(native._IP), cap
    buf = np.zeros(256, dtype=np.int8)
    p_in = buf.ctypes.data
    p_out = p_in if out_shift is None else p_in + out_shift
    if entry == "bds_blank_file":
        return lib.bds_blank_file(None, C.byref(cs), paths[0], paths[1], -1, piece, C.byref(o), C.byref(rep))
    return getattr(lib, entry)(None, C.byref(cs), C.c_void_p(p_in), n_bytes, C.c_void_p(p_out), C.byref(o), C.byref(rep))


def test_argument_checks_come_before_any_device_call(tmp_path):
    """Every argument error is BDS_ERR_ARG with a message, raised with no context at all (so no device call came before it)."""
    err = lambda: native.lib().bds_last_error(None).decode()
    for entry in ("bds_blank", "bds_blank_dev"):
        assert _call(entry, pre=-1) == -1 and "hold-off" in err()
        assert _call(entry, post=native.BLANK_MAX_WINDOW + 1) == -1 and "hold-off" in err()
        assert _call(entry, lead=40, tail=25) == -1 and "do not fit" in err()
        assert _call(entry, lead=-1) == -1 and "do not fit" in err()
        assert _call(entry, fmt="s8c", n_bytes=63) == -1 and "whole number of samples" in err()
        assert _call(entry, fmt="s16", n_bytes=63) == -1 and "whole number of samples" in err()
        assert _call(entry, fmt="s16c", n_bytes=62) == -1 and "whole number of samples" in err()
        assert _call(entry, ds=10, cap=6) == -1 and "holds 6 bins, the window takes 7" in err()
        assert _call(entry, ds=10) == -1 and "holds 0 bins" in err()
        assert _call(entry, ds=-1) == -1 and "duty_samples" in err()
        assert _call(entry, out_shift=16) == -1 and "overlap" in err()
        assert _call(entry, s=bc.settings_of("s8").copy(fileType=3)) < -1 and "no amplitude" in err()
        # valid arguments get as far as the missing context
        assert _call(entry) == -1 and "ctx is NULL" in err()
        assert _call(entry, ds=10, cap=7, out_shift=64) == -1 and "ctx is NULL" in err()
    assert _call("bds_blank_dev", fmt="s16", out_shift=65) == -1 and "aligned" in err()
    src, dst = tmp_path / "in.bin", tmp_path / "never_written.bin"
    np.zeros(100, dtype=np.int8).tofile(src)
    paths = (os.fsencode(src), os.fsencode(dst))
    assert _call("bds_blank_file", paths=paths, pre=30, post=20, piece=30) == -1 and "too small for its context" in err()
    assert _call("bds_blank_file", paths=paths, piece=-1) == -1 and "piece_samples" in err()
    assert _call("bds_blank_file", paths=paths, pre=-1) == -1 and "hold-off" in err()
    assert _call("bds_blank_file", paths=paths, lead=101) == -1 and "do not fit" in err()
    assert _call("bds_blank_file", paths=paths, ds=10, cap=9) == -1 and "holds 9 bins" in err()
    assert _call("bds_blank_file", paths=(paths[0], paths[0])) == -1 and "same file" in err()
    assert _call("bds_blank_file", paths=paths, s=bc.settings_of("s8", skipNumberOfBytes=101)) == -1 and "Could not read enough data" in err()
    assert _call("bds_blank_file", paths=paths) == -1 and "ctx is NULL" in err()
    assert not os.path.exists(dst)
    with pytest.raises(ValueError, match="threshold_sq"):
        native.pack_blank(2 ** 32, 1, 1)


def test_header_and_binding_name_the_same_entries():
    src = open(os.path.join(ROOT, "include", "bds_mi355x.h")).read()
    assert re.search(r"BDS_BLANK_DEV_API\s+int\s+bds_blank_dev\s*\(", src) and native.BLANK_DEVICE_EXPORTS == ["bds_blank_dev"]
    assert int(re.search(r"#define BDS_BLANK_TILE (\d+)", src).group(1)) == native.BLANK_TILE
    assert int(re.search(r"#define BDS_BLANK_MAX_WINDOW (\d+)", src).group(1)) == native.BLANK_MAX_WINDOW
    for entry in native.BLANK_DEVICE_EXPORTS + ["bds_blank", "bds_blank_file"]:
        assert hasattr(native.lib(), entry), entry
    assert callable(getattr(native.Context, "blank", None))
    assert C.sizeof(native.BlankOpts) == 40 and C.sizeof(native.BlankOut) == 56


def test_scene_needs_the_blanker(scene):
    """peakMetric of PRN 9 on the float64 oracle: 1.91 clean, 1.05 jammed, 1.77 blanked by the model (acqThreshold 1.5)"""
    s = scene.settings
    _, clean_rep = bc.model(scene.clean, "s8", scene.threshold ** 2, scene.pre, scene.post)
    assert clean_rep["n_flagged"] == 0 and clean_rep["n_blanked"] == 0
    blanked, rep = bc.model(scene.jammed, "s8", scene.threshold ** 2, scene.pre, scene.post)
    assert abs(rep["n_blanked"] / rep["n_samples"] - 0.250) <= 0.01
    assert np.array_equal(blanked[blanked != 0], scene.jammed[blanked != 0]) and rep["n_runs"] > 100
    jam = oacq.acquisition_b2a(scene.jammed.astype(np.float64), s)
    fix = oacq.acquisition_b2a(blanked.astype(np.float64), s)
    assert jam.carrFreq[8] == 0 and jam.peakMetric[8] < s.acqThreshold
    assert fix.carrFreq[8] != 0 and fix.peakMetric[8] >= s.acqThreshold + 0.25
    assert abs(fix.carrFreq[8] - (s.IF - 1230.0)) <= 50
