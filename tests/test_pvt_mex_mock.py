"""bds_mex('post_navigation', ...) through the stand-in MEX runtime of tests/test_mex_mock.py: what MATLAB's wrappers
(mex/B1C/postNavigation.m, mex/B2a/postNavigation.m) would hand over goes in; what comes back is what the ctypes path
(Context.post_navigation) gives on the same inputs, array for array."""
import math

import numpy as np
import pytest

import pvt_cases as pc
from bds_amd import native
from test_mex_mock import MexError, mex  # noqa: F401  (the fixture builds the gateway against the stand-in)

pytestmark = pytest.mark.gpu

SIG = {"B1C": 1, "B2A": 2}


def _eph_structs(mex, ephs):  # noqa: F811
    """1 x nCh struct array as 'nav_decode' returns eph: [] where NaN; None = an idle channel, every field []."""
    rows = []
    for e in ephs:
        d = {f: ([] if e is None or math.isnan(e[f]) else e[f]) for f in native.EPH_FIELDS}
        for f in ("SatType", "flag", "n_entered"):
            d[f] = [] if e is None else float(e[f])
        d["idValid"] = [] if e is None else np.asarray(e["idValid"], dtype=np.float64)
        rows.append(d)
    return mex.struct(rows)


def _call(mex, scn, status=None, ephs=None, settings=None, absolute_sample=None):  # noqa: F811
    s = settings or scn.settings
    a = scn.absoluteSample if absolute_sample is None else absolute_sample
    out, = mex.call(1, mex.value("post_navigation"), mex.settings(s), mex.double(SIG[scn.signal]), mex.value(status or scn.status),
                    mex.double(scn.prns), mex.double(a.reshape(-1)), mex.double(scn.codeFreq.reshape(-1)),
                    mex.double(scn.remCodePhase.reshape(-1)), _eph_structs(mex, ephs or scn.ephs), mex.double(scn.subFrameStart),
                    mex.double(scn.TOW))
    return {n: mex.doubles(mex.L.mxGetField(out, 0, n.encode())) for n in mex.fields(out)}


@pytest.mark.parametrize("name", ["b1c_5x7", "low_of_4", "b2a_6", "idle_and_no_eph"])
def test_post_navigation_through_the_gateway(ctx, mex, name):  # noqa: F811
    scn = pc.host_cases()[name]
    ephs = [None if st == "-" else e for st, e in zip(scn.status, scn.ephs)]
    got = _call(mex, scn, ephs=ephs)
    want, ready = ctx.post_navigation(scn.settings, scn.status, scn.prns, scn.absoluteSample, scn.codeFreq, scn.remCodePhase, scn.ephs,
                                      scn.subFrameStart, scn.TOW)
    n_meas = want["X"].size
    assert sorted(got) == sorted(pc.SOLUTION_FIELDS + ["n_meas", "ready"])
    assert got["n_meas"][0, 0] == n_meas and n_meas > 0
    np.testing.assert_array_equal(got["ready"][0], ready)
    for f in native.PVT_CHANNEL_FIELDS:
        assert got[f].shape == (scn.n_ch, n_meas), f
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)
    assert got["DOP"].shape == (5, n_meas)
    np.testing.assert_array_equal(got["DOP"], want["DOP"])
    for f in native.PVT_EPOCH_FIELDS:
        assert got[f].shape == (1, n_meas), f
        np.testing.assert_array_equal(got[f][0], want[f], err_msg=f)


def test_post_navigation_without_a_solution_and_error_exits(ctx, mex):  # noqa: F811
    scn = pc.host_cases()["b1c_5x7"]
    got = _call(mex, scn, status="T-T-T")
    assert got["n_meas"][0, 0] == 0 and list(got["ready"][0]) == [1, 2, 1, 2, 1]
    assert got["X"].size == 0 and got["PRN"].shape == (5, 0) and got["DOP"].shape == (5, 0)
    with pytest.raises(MexError, match="post_navigation: \\(settings, signal, status, PRN"):
        mex.call(1, mex.value("post_navigation"), mex.double(1))
    for name in native.PVT_SETTINGS:
        s = scn.settings.copy()
        delattr(s, name)
        with pytest.raises(MexError, match=f"settings.{name} is missing"):
            _call(mex, scn, settings=s)
    bad = scn.absoluteSample.copy()
    bad[2, 9] = bad[2, 8]
    with pytest.raises(MexError, match="strictly increasing"):
        _call(mex, scn, absolute_sample=bad)
    with pytest.raises(MexError, match="one column per channel"):
        mex.call(1, mex.value("post_navigation"), mex.settings(scn.settings), mex.double(1), mex.value(scn.status), mex.double(scn.prns),
                 mex.double(scn.absoluteSample.reshape(-1)[:-1]), mex.double(scn.codeFreq.reshape(-1)), mex.double(scn.remCodePhase.reshape(-1)),
                 _eph_structs(mex, scn.ephs), mex.double(scn.subFrameStart), mex.double(scn.TOW))
