"""MATLAB's colon operator as the oracle restates it (oracle/matlab.py m_colon, after MathWorks' published colonop.m): hand-worked
cases, and the C oracle's per-sample form (oracle/c/trk_oracle.c colon_at) against it on the reference's tcode vectors
(B2a/tracking.m:260-286, B1C/WB_tracking.m:289-317).  Also the CPU guards of tests/colon_states.py, the table of open-loop states
tests/test_track_colon_gpu.py runs the device correlators on: every state must be one on which the colon vector and a + k d really
part, or the GPU module would prove nothing."""
import ctypes

import numpy as np
import pytest

from oracle import cfast
from oracle.matlab import m_colon, m_colon_parts

import colon_states as cs


def test_known_matlab_elements():
    # 0:0.1:1 -- the textbook case: MATLAB's element 4 is 0.1*3 = 0.30000000000000004 (first half, a + k d), element 7 is
    # 1 - 4*0.1 = 0.6 (second half, from the right end; 6*0.1 = 0.6000000000000001 is NOT what MATLAB holds), the
    # mid-point (n = 10 even) is (0 + 1)/2
    v = m_colon(0.0, 0.1, 1.0)
    assert len(v) == 11
    assert v[3] == 0.1 * 3 == 0.30000000000000004
    assert v[5] == 0.5
    assert v[6] == 1.0 - 4 * 0.1 and v[6] != 6 * 0.1
    assert v[7] == 1.0 - 3 * 0.1 and v[8] == 1.0 - 2 * 0.1 and v[9] == 1.0 - 0.1 and v[10] == 1.0


def test_odd_n_has_no_midpoint_and_halves_are_disjoint():
    # n = 9 intervals (10 elements): 0..4 from the left, 5..9 from the right
    a, d, b = 0.1, 0.1, 1.0
    n, c = m_colon_parts(a, d, b)
    assert n == 9 and c == b
    v = m_colon(a, d, b)
    for k in range(5):
        assert v[k] == a + k * d
        assert v[9 - k] == c - k * d


def test_right_end_is_snapped_only_within_tolerance():
    # a + n d one ulp away from b: snapped (c == b exactly)
    a, d = 0.3, 0.1
    b = np.nextafter(a + 7 * d, 2.0)
    n, c = m_colon_parts(a, d, b)
    assert n == 7 and c == b
    # b well short of a + n d: that element is not produced, and the end is NOT b
    n, c = m_colon_parts(0.0, 0.3, 1.0)
    assert n == 3 and c == 0.0 + 3 * 0.3 and c != 1.0
    # round() up, then the overshoot rule takes the last interval back: (b-a)/d = 2.6 -> round 3 -> 0.9 > 0.8 + tol -> n = 2
    n, c = m_colon_parts(0.0, 0.3, 0.8)
    assert n == 2 and c == 0.0 + 2 * 0.3


def test_empty_and_integer_branches():
    assert len(m_colon(1.0, 0.1, 0.5)) == 0
    np.testing.assert_array_equal(m_colon(0.0, 1.0, 7.0), np.arange(8.0))
    np.testing.assert_array_equal(m_colon(2.0, 3.0, 12.5), np.array([2.0, 5.0, 8.0, 11.0]))


@pytest.mark.parametrize("scale,spc,code_len", [(1.0, 0.5, 10230.0), (2.0, 0.25, 10230.0)], ids=["b2a", "b1c"])
def test_c_per_sample_form_is_the_vector(scale, spc, code_len):
    """the C oracle evaluates element k on the fly; the NumPy oracle builds the whole vector: same doubles, and the diagnostic
    counter agrees with a direct count of the ceil() differences against a + k d"""
    cfast.build()
    L = cfast.lib()
    L.bds_oracle_trk_colon_diff.argtypes = [ctypes.c_long] + [ctypes.c_double] * 4 + [ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_double)]
    L.bds_oracle_trk_colon_diff.restype = ctypes.c_int
    rng = np.random.default_rng(5)
    fs = 99.375e6
    for trial in range(40):
        code_freq = (1.023e6 if scale == 2.0 else 10.23e6) * (1 + rng.uniform(-3e-6, 3e-6))
        step = code_freq / fs
        rem = rng.uniform(0, step) if trial else 0.0
        blk = int(np.ceil((code_len - rem) / step))
        _c_form_is_the_vector(L, blk, rem, step, spc, scale)


def _c_form_is_the_vector(L, blk, rem, step, spc, scale):
    counts = (ctypes.c_long * 6)()
    mu = ctypes.c_double()
    assert L.bds_oracle_trk_colon_diff(blk, rem, step, spc, scale, counts, ctypes.byref(mu)) == 0
    kk = np.arange(blk, dtype=np.float64)
    for r, off in enumerate((-spc, 0.0, spc)):
        t = m_colon((rem + off) * scale, step * scale, (((blk - 1) * step + rem) + off) * scale)
        assert len(t) == blk
        plain = (rem + off) * scale + kk * (step * scale)
        assert np.all(np.diff(t) > 0)
        assert counts[r] == int(np.count_nonzero(np.ceil(t) != np.ceil(plain)))
        assert counts[3 + r] == int(np.count_nonzero(np.ceil(t * 6) != np.ceil(plain * 6)))
        # the first half IS a + k d; the second half is within a few ulp of it
        h = (blk - 1) // 2
        np.testing.assert_array_equal(t[:h], plain[:h])
        assert np.max(np.abs(t - plain)) <= 4 * np.spacing(t[-1])
    assert 0 <= mu.value <= 4
    return [int(c) for c in counts]


_IDS = [s.name for s in cs.STATES]


@pytest.mark.parametrize("st", cs.STATES, ids=_IDS)
def test_colon_states_are_adversarial(st):
    """every state of the table the GPU module runs: (1) >= 100 samples whose index differs between the colon vector and a + k d, in
    an index the state's mode reads (C oracle's counter); (2) the NumPy oracle's vector and the C oracle's per-sample form agree on
    the state; (3) on the record the GPU test uses, the C oracle's sums in the two forms differ by >= 1e-3 of |P| in a sum the mode
    reports -- 1000 x the open-loop tolerance.  All oracle against oracle."""
    read = cs.counts_read(st)
    counts = _c_form_is_the_vector(cs._trk_lib(), cs.blk_of(st), st.rem, cs.step_of(st), st.spacing, 1.0 if st.signal == "B2A" else 2.0)
    assert counts == cs.colon_counts(st)
    x, chans = cs.record_of(st)
    colon, plain = cs.oracle_sums(st, x, chans), cs.oracle_sums(st, x, chans, plain=True)
    n = cs.n_sums(st)
    gap = np.abs(colon[:, :n] - plain[:, :n]).max(axis=1) / np.hypot(colon[:, 2], colon[:, 3])
    assert np.array_equal(cs.oracle_sums(st, x, chans), colon)  # the plain form was switched off again
    if st.counted:
        assert max(read) >= 100, read
        assert gap.min() >= 1e-3, gap  # every channel of the record
    else:
        assert 0 < max(read) < 100 and gap.max() > 0
    # a real correlation peak: the prompt sum stands well above the early / late ones' difference from it
    assert np.all(np.hypot(colon[:, 2], colon[:, 3]) > 50 * np.sqrt(cs.blk_of(st)))
    if "-h-" in st.name:
        assert cs.junction_place(st)[3], "the block length does not put the junction where the name says"


def test_colon_state_table_covers_what_it_claims():
    c = [s for s in cs.STATES if s.counted]
    assert {(s.signal, s.mode) for s in c} == {("B2A", "B2A"), ("B1C", "NB"), ("B1C", "WB")}
    for mode in ("B2A", "NB", "WB"):
        assert {s.iq for s in c if s.mode == mode} == {False, True}
    diff = {s.name: cs.colon_counts(s) for s in c}
    assert any(v[1] >= 100 and v[0] == 0 and v[2] == 0 for v in diff.values())  # the prompt replica alone
    assert any(min(v[:3]) >= 100 for v in diff.values())  # early and late as well
    assert any(max(v[:3]) == 0 and v[4] >= 100 for s, v in zip(c, diff.values()) if s.mode == "WB")  # the BOC(6,1) index alone
    assert any(v[0] >= 100 and v[3] >= 100 and v[5] >= 100 for s, v in zip(c, diff.values()) if s.mode == "WB")  # wide-band early / late
    assert {(cs.blk_of(s) - 1) % 2 for s in c} == {0, 1}
    assert any(s.fs == 99.375e6 and s.signal == "B2A" for s in c) and any(s.fs == 99.375e6 and s.signal == "B1C" for s in c)
    places = {cs.junction_place(s)[:3] for s in c if "-h-" in s.name}
    assert places == {(w, e, p) for w in ("chunk", "pass", "seg") for e in ("first", "last") for p in ("even", "odd")}
    assert any(cs.blk_of(s) % 16 not in (0, 1, 15) and cs.blk_of(s) < 0.5 * cs.nominal_blk(s) for s in c)  # ends inside a segment


@pytest.mark.parametrize("st", cs.QUIET, ids=[s.name for s in cs.QUIET])
def test_the_guard_rejects_a_state_off_the_lattice(st):
    """the same rates with a code phase off the boundary lattice: no differing sample, identical sums -- such a row in the table would
    fail test_colon_states_are_adversarial"""
    assert cs.colon_counts(st) == [0] * 6
    x, chans = cs.record_of(st)
    np.testing.assert_array_equal(cs.oracle_sums(st, x, chans), cs.oracle_sums(st, x, chans, plain=True))


def test_oracle_refuses_a_spacing_whose_indices_leave_the_code_arrays():
    """wide-band mode with a quarter-chip spacing: ceil(tcode * 6) + 1 of the early replica starts at -2 and that of the late one ends
    past [p(end) p p(1)] -- MATLAB stops with an index error there (WB_tracking.m:298,324); the C sample loop would read outside its
    arrays, so its front raises first"""
    st = cs.STATES[0]._replace(spacing=0.25)
    assert st.mode == "WB"
    x, chans = cs.record_of(st)
    with pytest.raises(IndexError, match="outside the padded code array"):
        cs.oracle_sums(st, x, chans)
    cs.oracle_sums(st._replace(spacing=1.0 / 12.5), x, chans)  # inside 1 / 12 chip: fine
