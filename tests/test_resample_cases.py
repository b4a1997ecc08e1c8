"""The cases, references and tolerances of tests/resample_cases.py are what tests/test_resample_stages_gpu.py and
tests/test_resample_block_gpu.py take them for -- checked on the CPU, before a GPU sees them: the references compose to scipy's filtfilt and
the oracle's resample_condition, a plain float64 evaluation lies well inside the derived tolerance, the decimation cases contain the
samples on which the neighbouring evaluation orders part from the reference, and NumPy models of the kernels with ONE change each fail
the very assertion functions the GPU tests call (the unchanged models pass all of them)."""
import numpy as np
import pytest

import resample_cases as rc

T = 701


def report(name, value):
    print(f"\nresample_cases: {name} = {value:.3e}")


def test_long_double_carries_64_bits_and_double_double_agrees():
    assert np.finfo(np.longdouble).nmant >= 63
    g = rc.fir_group("asym", 257, 771)
    for u in g.signals[:3]:
        hi, lo = rc.pass_ref_dd(u, g.b)
        err = np.abs((hi.astype(np.longdouble) + lo) - rc.pass_ref(u, g.b)).astype(np.float64)
        assert np.all(err <= 257 * 2.0 ** -63 * rc.pass_abs(u, g.b))  # the long-double chain's own bound: the two agree to its last bits


def test_extension_is_the_literal_expression_and_scipys_odd_extension():
    from scipy.signal._arraytools import odd_ext

    for c in rc.extend_cases()[:10]:
        x = c.x.astype(np.int64)
        n, nfact = len(x), c.nfact
        one = lambda i: x[i - 1]  # noqa: E731  (MATLAB's 1-based x(i))
        lit = np.concatenate([[2 * one(1) - one(i) for i in range(nfact + 1, 1, -1)], x, [2 * one(n) - one(i) for i in range(n - 1, n - nfact - 1, -1)]])
        ref = rc.extend_ref(x, nfact)
        assert np.array_equal(ref, lit) and np.array_equal(ref, odd_ext(x, nfact, axis=0)) and len(ref) == n + 2 * nfact


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_references_compose_to_scipy_filtfilt_and_the_oracle(cplx):
    """extend, pass, reverse pass, decimate = scipy.signal.filtfilt(b, 1, x, padtype='odd', padlen=2100) + the oracle's index selection =
    oracle.acquisition.resample_condition, within tol2 (scipy's passes are float64 chains of the same length)."""
    import scipy.signal as ssig

    import bds_amd
    from oracle import acquisition as oacq

    s = bds_amd.init_settings_b2a(resamplingflag=1)
    rng = np.random.default_rng(110)
    n = 110000
    xi, xq = (np.clip(np.round(30 * rng.standard_normal(n)), -128, 127).astype(np.int8) for _ in range(2))
    fs, bw = s.samplingFreq, s.codeFreqBasis * 2 + 0.5e6
    wp = [(s.IF - bw / 2) * 2 / fs - 0.002, (s.IF + bw / 2) * 2 / fs + 0.002]
    b = ssig.firwin(T, wp, window="hamming", pass_zero=False, scale=True)
    new_fs = rc.plan_rates(fs, s.IF, bw)
    x = xi.astype(np.float64) + 1j * xq if cplx else xi.astype(np.float64)
    got, s2, old = oacq.resample_condition(x, s)
    assert s2.samplingFreq == new_fs == 48.06e6 and old == (fs, s.IF)
    full = ssig.filtfilt(b, [1.0], x, padtype="odd", padlen=3 * (T - 1))
    worst = 0.0
    for part, xs in ((np.real, xi), (np.imag, xq))[:2 if cplx else 1]:
        r = rc.filtfilt_ref(xs, b, new_fs, fs)
        assert len(r.ref) == len(got) == rc.sig_len_of(n, new_fs, fs)
        assert np.array_equal(part(got), part(full)[r.idx - 1])  # the oracle's selection
        worst = max(worst, rc.worst_ratio(part(got), r.ref, r.tol))
        report("largest |scipy - reference|", float(np.max(np.abs(part(got) - r.ref))))
    report("scipy filtfilt: largest error / tol2", worst)


def test_plain_float64_lies_well_inside_tol1():
    """A sequential float64 evaluation without FMA of the library's shortest extended block (6301 samples, 701 taps): inside the bound,
    and not by so much that the bound says nothing (it reaches 0.02 of it)."""
    worst = 0.0
    for kind in ("fir1", "asym"):
        g = rc.fir_group(kind, T, rc.FIR_MIN_LEN)
        for i in (0, 1):
            y = rc.model_fir(g.signals[i][:, None], g.b, 0)[:, 0]
            worst = max(worst, rc.worst_ratio(y, rc.pass_ref(g.signals[i], g.b), rc.tol1_of(g.signals[i], g.b)))
    report("sequential float64: largest error / tol1", worst)
    assert 1e-3 < worst < 0.5


def test_taps_and_plan():
    import scipy.signal as ssig

    import bds_amd
    from bds_amd import native

    for n in rc.FIR_TAPS:
        b, a = rc.taps_of("fir1", n), rc.taps_of("asym", n)
        assert len(b) == len(a) == n and rc.same_bits(b, b[::-1])
        assert not np.any(a[:n // 2] == a[::-1][:n // 2])  # no tap equals its mirror: a reversed tap order changes every product
        if n >= 3:
            ref = ssig.firwin(n, [0.0648805, 0.4845195], window="hamming", pass_zero=False, scale=True)
            np.testing.assert_allclose(b, ref, rtol=0, atol=4e-16 * np.abs(ref).max() * n)
    assert rc.fir_lengths(701) == [1, 700, 701, 702, 2103, 6301] and rc.fir_lengths(1) == [1, 2, 3, 6301]
    for s, want in ((bds_amd.init_settings_b1c(resamplingflag=1), rc.B1C_53_NEW_FS), (bds_amd.init_settings_b2a(resamplingflag=1), 48.06e6),
                    (bds_amd.init_settings_b1c(samplingFreq=99.375e6, IF=14.58e6, resamplingflag=1), 19.62e6),
                    (bds_amd.init_settings_b1c(samplingFreq=40e6, IF=10e6, resamplingflag=1, resamplingThreshold=15e6), 29e6)):
        assert native.resample_plan(s)[0] == want
    assert {(o, n) for o, n, _, _ in rc.DEC_PAIRS} == {(40e6, 29e6), (99.375e6, 19.62e6), (99.375e6, 48.06e6), (53e6, rc.B1C_53_NEW_FS)}


def test_decimation_cases_contain_the_other_evaluation_orders():
    """float64's ceil((k / fs') fs) is not the exact ceiling, and each neighbouring evaluation order parts from it inside every case (at
    the k listed in resample_cases.DEC_PAIRS)."""
    from fractions import Fraction

    firsts = {(40e6, 29e6): (87, 145, 29), (99.375e6, 19.62e6): (22236, 22236, 11772), (99.375e6, 48.06e6): (54468, 54468, 16020)}
    for old, new, n, named in rc.DEC_PAIRS[:3]:
        ref = rc.decimate_index(n, new, old)
        others = rc.other_orders(n, new, old)
        first = tuple(int(np.nonzero(others[k] != ref)[0][0]) for k in ("k*(old/new)", "k*old/new", "k*(1/new)*old"))
        assert first == firsts[(old, new)] and set(first) <= set(named) and max(named) < n
        ratio = Fraction(int(old)) / Fraction(int(new))
        exact = np.array([1] + [-((-k * ratio.numerator) // ratio.denominator) for k in range(1, n)])
        assert np.any(exact != ref)  # (the reference is float64's, as MATLAB's and the oracle's: not the exact ceiling)
    big = rc.decimate_cases()[-1]
    assert big.sig_len > 2048 * 256 and all(np.any(v != rc.decimate_index(big.sig_len, big.new_fs, big.old_fs))
                                            for v in rc.other_orders(big.sig_len, big.new_fs, big.old_fs).values())


def test_decimation_never_selects_past_the_end_of_the_block():
    for old, new, _, _ in rc.DEC_PAIRS:
        for n_in in list(range(2101, 2400)) + list(range(198700, 198900)) + list(range(800000, 800040)) + [400001, 530000, 1987500]:
            m = rc.sig_len_of(n_in, new, old)
            if m >= 1:
                assert rc.decimate_index(m, new, old).max() <= n_in, (old, new, n_in)
    for c in rc.decimate_cases():  # and the cases' inputs hold every index of the reference and of its three neighbours
        zlen = len(rc.decimate_input(c))
        assert max(v.max() for v in rc.other_orders(c.sig_len, c.new_fs, c.old_fs).values()) + c.nfact <= zlen
    for need, new, old in ((96120, 48.06e6, 99.375e6), (580000, 29e6, 40e6)):
        n = rc.shortest_input(need, new, old)
        assert rc.sig_len_of(n, new, old) >= need > rc.sig_len_of(n - 1, new, old)
    assert rc.shortest_input(96120, 48.06e6, 99.375e6) == 198751


# ---- the assertions bite -------------------------------------------------------------------------------------------------------
def extend_all(mutant=None):
    for c in rc.extend_cases():
        rc.assert_extend(c, rc.model_extend(c.x, c.nfact, mutant))


def decimate_all(mutant=None):
    for c in rc.decimate_cases():
        rc.assert_decimate(c, rc.model_decimate(rc.decimate_input(c), c.nfact, c.sig_len, c.new_fs, c.old_fs, mutant))


def fir_some(kind, mutant=None, taps=(2, 257, T)):
    worst = 0.0
    for n in taps:
        for g in rc.fir_groups(n):
            if g.name.startswith(kind):
                worst = max(worst, rc.assert_fir_group(g, rc.model_group(g, mutant)))
    return worst


def test_the_unchanged_models_pass_every_assertion():
    extend_all()
    decimate_all()
    for x in rc.widen_cases():
        rc.assert_widen(x, x.astype(np.float64))
    worst = max(rc.assert_fir_group(g, rc.model_group(g)) for n in rc.FIR_TAPS for g in rc.fir_groups(n))
    report("models, every FIR group: largest error / tol1", worst)


# mutant -> the check that must reject it.  'fir1' / 'asym': assert_fir_group on the groups with those taps.
MUTANTS = (("taps in the other direction", "asym"),
           ("forward and reverse pass exchanged", "asym"),
           ("clamp to u(1)", "fir1"),
           ("clamp to u(1)", "asym"),
           ("steady-state start replaced by zeros", "fir1"),
           ("steady-state start replaced by zeros", "asym"),
           ("head reflection without 2 x(0)", "extend"),
           ("tail reflection shifted by one", "extend"),
           ("I and Q exchanged", "extend"),
           ("I and Q exchanged", "fir1"),
           ("I and Q exchanged", "decimate"),
           ("floor for ceil", "decimate"),
           ("k == 0 rule dropped", "decimate"),
           ("k*(old/new)", "decimate"),
           ("k*old/new", "decimate"),
           ("k*(1/new)*old", "decimate"))


@pytest.mark.parametrize("mutant, check", MUTANTS, ids=[f"{m} [{c}]" for m, c in MUTANTS])
def test_a_model_with_one_change_fails(mutant, check):
    with pytest.raises(AssertionError) as e:
        if check == "extend":
            extend_all(mutant)
        elif check == "decimate":
            decimate_all(mutant)
        else:
            fir_some(check, mutant)
    print(f"\nresample_cases: '{mutant}' rejected by {check}: {str(e.value)[:160]}")


def test_symmetric_taps_hide_what_asymmetric_taps_show():
    """Why the cases carry asymmetric taps: with fir1's taps (b == flip(b) to the bit) a tap order run backwards, or the two passes
    exchanged, still lies within the tolerance of every output."""
    for mutant in ("taps in the other direction",):
        assert fir_some("fir1", mutant, taps=(257,)) <= 1.0


def test_each_evaluation_order_fails_on_each_rate_pair():
    """(The dropped k == 0 rule reads z[nfact - 1]: with nfact = 0 that is the element in FRONT of z, which the model takes for z[0] and
    the driver keeps inside its allocation, prefilled with the NaN pattern -- so only the cases with nfact = 2100 are asked for here.)"""
    for c in rc.decimate_cases():
        if c.new_fs == rc.B1C_53_NEW_FS:
            continue
        for mutant in ("k*(old/new)", "k*old/new", "k*(1/new)*old", "floor for ceil") + (("k == 0 rule dropped",) if c.nfact else ()):
            with pytest.raises(AssertionError):
                rc.assert_decimate(c, rc.model_decimate(rc.decimate_input(c), c.nfact, c.sig_len, c.new_fs, c.old_fs, mutant))


def test_case_file_and_output_guard(tmp_path):
    c = rc.extend_cases()[-1]
    arrays = rc.case_file([rc.job_extend(c), rc.job_widen(rc.widen_cases()[1])])
    rc.write_arrays(str(tmp_path / "case.bin"), arrays)
    back = rc.read_arrays(str(tmp_path / "case.bin"))
    assert len(back) == 5 and back[0].view(np.int64).tolist() == [rc.MAGIC, 2] and np.array_equal(back[2].view(np.int16).reshape(c.x.shape), c.x)
    assert np.isnan(np.array([rc.FILL], dtype=np.uint64).view(np.float64)[0])
    raw = np.full(10 + rc.GUARD, rc.FILL, dtype=np.uint64)
    raw[:10] = np.arange(10.0).view(np.uint64)
    assert np.array_equal(rc.split_output(raw.view(np.uint8), (5, 2)).ravel(), np.arange(10.0))
    for spoil in (3, 10, 10 + rc.GUARD - 1):  # an element never written; the first and the last guard word written
        bad = raw.copy()
        bad[spoil] = rc.FILL if spoil < 10 else 0
        with pytest.raises(AssertionError):
            rc.split_output(bad.view(np.uint8), (5, 2))
