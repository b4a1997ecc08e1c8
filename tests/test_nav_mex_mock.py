"""bds_mex('nav_decode', ...) through the stand-in MEX runtime of tests/test_mex_mock.py: what MATLAB's wrappers
(mex/B1C/include/BCNAV1decoding.m, mex/B2a/include/BCNAV2decoding.m) would hand over goes in; what comes back is what the
ctypes path (Context.nav_decode) gives on the same prompts."""
import math

import numpy as np
import pytest

import bds_amd
import nav_cases as nc
from bds_amd import native
from test_mex_mock import MexError, mex  # noqa: F401  (the fixture builds the gateway against the stand-in)

pytestmark = pytest.mark.gpu


def _struct(mex, a):  # noqa: F811
    return {n: mex.L.mxGetField(a, 0, n.encode()) for n in mex.fields(a)}


def _same(mex, out, want):  # noqa: F811
    top = _struct(mex, out)
    eph = _struct(mex, top["eph"])
    assert sorted(eph) == sorted(native.EPH_FIELDS + ["SatType", "flag", "n_entered", "idValid"])
    for f in native.EPH_FIELDS:
        v = mex.doubles(eph[f])
        if math.isnan(want["eph"][f]):
            assert v.size == 0, f
        else:
            assert v.shape == (1, 1) and v[0, 0] == want["eph"][f], f
    for f in ("SatType", "flag", "n_entered"):
        assert mex.doubles(eph[f])[0, 0] == want["eph"][f]
    np.testing.assert_array_equal(mex.doubles(eph["idValid"])[0], want["eph"]["idValid"])
    assert mex.doubles(top["firstSubFrame"])[0, 0] == want["firstSubFrame"] and mex.doubles(top["TOW"])[0, 0] == want["TOW"]
    assert mex.doubles(top["n_frames"])[0, 0] == want["n_frames"]
    for f in ("index", "status", "polarity"):
        col = mex.doubles(top[f])
        assert col.shape == (want["n_frames"], 1)
        np.testing.assert_array_equal(col[:, 0], [fr[f] for fr in want["frames"]])


def test_nav_decode_through_the_gateway(ctx, mex):  # noqa: F811
    rng = np.random.default_rng(51)
    _, s1 = nc.b1c_message(rng, 23, 1)
    _, s3 = nc.b1c_message(rng, 23, 3)
    pilot = nc.b1c_pilot(rng, 3700, 23, [37, 1837])
    data = nc.noise_like(rng, 3700)
    nc.place(data, 37, s1, rng, -1.0)
    nc.place(data, 1837, s3, rng)
    out, = mex.call(1, mex.value("nav_decode"), mex.double(1), mex.double(23), mex.double(pilot), mex.double(data))
    want = ctx.nav_decode(bds_amd.init_settings_b1c(), [23], pilot[None], data[None], cap=64)[0]
    assert want["eph"]["n_entered"] == 2 and want["firstSubFrame"] == 37
    _same(mex, out, want)

    _, sym = nc.b2a_message(rng, 31, 30)
    ip = nc.noise_like(rng, 3100)
    nc.place(ip, 45, sym, rng)
    out, = mex.call(1, mex.value("nav_decode"), mex.double(2), mex.double(1), mex.double(ip), mex.double([]))
    want = ctx.nav_decode(bds_amd.init_settings_b2a(), [1], ip[None], cap=64)[0]
    assert want["eph"]["idValid"][2] == 30 and want["firstSubFrame"] == 45
    _same(mex, out, want)
    # nothing to find: inf, every field []
    x = nc.noise_like(rng, 500)
    out, = mex.call(1, mex.value("nav_decode"), mex.double(2), mex.double(1), mex.double(x), mex.double([]))
    want = ctx.nav_decode(bds_amd.init_settings_b2a(), [1], x[None], cap=64)[0]
    assert want["n_frames"] == 0 and math.isinf(want["TOW"])
    _same(mex, out, want)


def test_nav_decode_error_exits(ctx, mex):  # noqa: F811
    with pytest.raises(MexError, match="nav_decode: \\(signal, PRN, sync_bits, data_bits\\)"):
        mex.call(1, mex.value("nav_decode"), mex.double(1), mex.double(5))
    with pytest.raises(MexError, match="differ in length"):
        mex.call(1, mex.value("nav_decode"), mex.double(1), mex.double(5), mex.double(np.ones(1800)), mex.double(np.ones(7)))
    with pytest.raises(MexError, match="PRN 64 out of range"):
        mex.call(1, mex.value("nav_decode"), mex.double(1), mex.double(64), mex.double(np.ones(1800)), mex.double(np.ones(1800)))
    with pytest.raises(MexError, match="settings.signal invalid"):
        mex.call(1, mex.value("nav_decode"), mex.double(3), mex.double(5), mex.double(np.ones(1800)), mex.double([]))
