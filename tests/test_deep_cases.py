"""The NumPy model of the weak-signal acquisition rule (tests/deep_cases.py) on its own, no GPU: it is the reference's search at
K = 1, it finds what the reference misses, the block alignment matters, five deliberate changes of the rule are told apart by the
tolerances the GPU tests use, and no GPU scene turns on a near-tie.  Figures of the scenes (model, float64):

  B2a 25 MS/s, K = 16   PRN 9 (46 dB-Hz)  reference peakMetric 2.31, deepMetric 33.8
                        PRN 14 (36 dB-Hz) reference 1.17 (missed), bin 8, codePhase 20323, deepMetric 3.73 (K = 1: 1.05)
                        PRN 21 (absent)   reference 1.11, deepMetric 1.03
  B1C 12.5 MS/s, K = 8  PRN 12 (35 dB-Hz) reference 6.39 < 7.5 (missed), deepMetric 7.64; PRN 7 (absent) 1.07
The 12 MS/s and 5 MS/s scenes (plan matrix, shifts, peaks at the ends of the surface, bin chunks) carry theirs in their docstrings.
"""
import os

import numpy as np
import pytest

import deep_cases as dc
from oracle import acquisition as oacq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("scene", ["mixed_b2a", "mixed_b1c"])
def test_one_block_is_the_reference(scene):
    s, x, _ = dc.GPU_SCENES[scene]()
    diag = {}
    ref = oacq.acquisition(dc.as_samples(x, s), s, diag)
    m = dc.model(x, s, 1, dc.THRESHOLD)
    for p, r in m.items():
        assert (r.fbin, r.codePhase) == (diag[p]["fbin"], diag[p]["codePhase"])
        np.testing.assert_allclose(r.peakMetric, ref.peakMetric[p - 1], rtol=1e-12)
    if scene == "mixed_b2a":
        assert m[14].deepMetric < 1.25  # one block does not find the weak one


def test_mixed_b2a_finds_the_weak_satellite():
    s, x, k = dc.mixed_b2a()
    ref = oacq.acquisition(dc.as_samples(x, s), s)
    assert ref.carrFreq[8] != 0 and ref.carrFreq[13] == 0 and ref.carrFreq[20] == 0
    assert ref.peakMetric[13] < s.acqThreshold
    m = dc.scene_model("mixed_b2a")
    assert m[9].deepMetric >= 2 and m[14].deepMetric >= 2 and m[21].deepMetric <= 1.25
    assert (m[14].fbin, m[14].codePhase) == (8, 20323) and abs(m[14].carrFreq - (s.IF + 830)) <= 50
    assert [m[p].detected for p in (9, 14, 21)] == [True, True, False]


def test_mixed_b1c_finds_the_weak_satellite():
    s, x, k = dc.mixed_b1c()
    ref = oacq.acquisition(dc.as_samples(x, s), s)
    assert not ref.carrFreq.any() and ref.peakMetric[11] < s.acqThreshold
    m = dc.scene_model("mixed_b1c")
    assert m[12].deepMetric >= 2 and m[12].detected and m[7].deepMetric <= 1.25 and not m[7].detected
    assert m[12].codePhase == 99002 + 1 and abs(m[12].carrFreq - (s.IF - 110)) <= 25


def _high_doppler(compensate, sign=1):
    s, x, k = dc.high_doppler_b2a()
    surf, _, bins = dc.surface(dc.as_samples(x, s), s, 14, k, compensate, bins=range(46, 51), sign=sign)
    d = dc.decide(surf, s)
    return bins[d.fbin], d.l0, d.deepMetric


def test_high_doppler_needs_the_alignment():
    """+9170 Hz: 0.195 samples of code drift per period, 11.7 over 60 blocks.  Aligned per bin the peak stands at the first
    block's lag; unaligned (or aligned with the wrong sign) it is smeared and found early."""
    b, l0, dm = _high_doppler(True)
    assert (b, l0) == (48, 20322) and dm >= 2
    _, l0_off, dm_off = _high_doppler(False)
    assert l0_off != 20322 and dm_off < dm
    _, l0_neg, dm_neg = _high_doppler(True, sign=-1)
    assert l0_neg != 20322 and dm_neg < dm_off


def test_changed_rules_are_told_apart():
    """One deliberate change each; the difference to the rule is far outside what the GPU tests allow."""
    # the sign of sh: the surface-value tolerance of the wrap scene
    s, x, k = dc.wrap_b2a()
    r = dc.scene_model("wrap_b2a")[9]
    wrong, _, _ = dc.surface(dc.as_samples(x, s), s, 9, k, sign=-1)
    assert np.max(np.abs(wrong - r.surface)) > 100 * r.tol
    # one tile of the column pass skipped (the surface keeps what it held) or run twice in one block: the values of that block at
    # the tile's lags n1 L2 + col are missing or doubled.  The smallest tile of the plan matrix (tests/test_deep_plans_gpu.py): the
    # last one of 8 x 4500, 4 columns x 5 rows inside N -- in every bin and every block
    s, x, k = dc.plans_b2a()
    r = dc.scene_model("plans_b2a")[9]
    (t, tiles, last), l2, n = dc.PLANS_B2A["8x4500"], 4500, dc.sizes(s)[2]
    lags = np.array([n1 * l2 + (tiles - 1) * t + j for n1 in range(8) for j in range(last)])
    lags = lags[lags < n]
    assert lags.size == 20
    for kk in range(k):
        rows = dc.block_rows(dc.as_samples(x, s), s, 9, kk)
        assert min(float(np.max(row[lags] ** 2)) for row in rows.values()) > 100 * r.tol
    # amplitude sums instead of power sums: another surface, and a worse statistic for the weak satellite
    s, x, k = dc.mixed_b2a()
    r = dc.scene_model("mixed_b2a")[14]
    amp, _, _ = dc.surface(dc.as_samples(x, s), s, 14, k, power=False)
    assert np.max(np.abs(amp - r.surface)) > 100 * r.tol
    assert dc.decide(amp, s).deepMetric < r.deepMetric
    # a population that forgets the images one code period away: the image of a strong peak becomes S_sec
    r9 = dc.scene_model("mixed_b2a")[9]
    d = dc.decide(r9.surface, s, images=False)
    assert abs(d.deepMetric - r9.deepMetric) > 100 * dc.deep_metric_bound(r9) and d.deepMetric < 2
    # the fine weights
    s, x, k = dc.mixed_b1c()
    r = dc.scene_model("mixed_b1c")[12]
    f = dc.fine(dc.as_samples(x, s), s, 12, k, r.codePhase - 1, r.fbin - 1, weights=(1.0, 1.0))
    assert np.max(np.abs(f - r.F)) > 1e-6 * r.F.max()


@pytest.mark.parametrize("name", sorted(dc.GPU_SCENES))
def test_no_gpu_scene_turns_on_a_near_tie(name):
    """S_peak - S_sec of every PRN of every scene the GPU tests use is above 100 x the surface tolerance."""
    for prn, r in dc.scene_model(name).items():
        print(f"\n{name} PRN {prn}: deepMetric {r.deepMetric:.3f}, margin / tolerance {r.margin / r.tol:.0f}")
        assert r.margin > 100 * r.tol, (name, prn)


def test_noise_floor_table():
    """profiles/deep_noise_floor.txt (tools/deep_noise_floor.py: K = 1, 4, 16, 64, 20 seeds, B2a D = 11 and B1C D = 9): every
    noise-only value lies above 1 by construction and below the threshold the tests run with; its first B2a rows are recomputed
    here for three seeds."""
    rows = [ln.split() for ln in open(os.path.join(ROOT, "profiles", "deep_noise_floor.txt")) if ln.strip().startswith("K =")]
    assert [int(r[2]) for r in rows] == [1, 4, 16, 64] * 2
    lo, hi = min(float(r[3]) for r in rows), max(float(r[7]) for r in rows)
    assert 1.0 <= lo and hi < dc.THRESHOLD
    got = dc.noise_floor(dc.b2a_settings([21]), (1, 4), range(100, 103))
    for k, row in zip((1, 4), rows):
        assert all(float(row[3]) - 5e-4 <= v <= float(row[7]) + 5e-4 for v in got[k]), (k, got[k], row)


def test_abi_surface():
    """The header declares the five entries, the ctypes mirror lists them and the library exports them; bds_deep_opts has the
    header's layout."""
    import ctypes
    import re

    from bds_amd import native

    src = open(os.path.join(ROOT, "include", "bds_mi355x.h")).read()
    for entry in ("bds_acq_deep", "bds_acq_deep_row", "bds_acq_deep_fine", "bds_acq_deep_release"):
        assert re.search(r"BDS_API\s+int\s+%s\s*\(" % entry, src) and entry in native.EXPORTS and hasattr(native.lib(), entry), entry
    assert re.search(r"BDS_DEEP_DEV_API\s+int\s+bds_acq_deep_dev\s*\(", src) and native.DEEP_DEVICE_EXPORTS == ["bds_acq_deep_dev"]
    assert hasattr(native.lib(), "bds_acq_deep_dev")
    assert re.search(r"int32_t n_blocks;.*\n\s*int32_t compensate;.*\n\s*int32_t keep_surface;\n\s*double threshold;.*\n\s*double surface_gib;", src)
    assert ctypes.sizeof(native.DeepOpts) == 32 and native.DeepOpts.threshold.offset == 16
