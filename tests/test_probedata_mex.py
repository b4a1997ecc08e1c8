"""bds_mex('probe_data', ...) EXECUTED against the stand-in for the MEX runtime (tests/mex_stub, as tests/test_mex_mock.py does for
the other commands): argument checks, the fields and shapes mex/probeData.m reads, and the numbers against bds_amd.probe_data on
the same file.  mex/probeData.m itself needs MATLAB to run; here it is held to the fields the gateway returns."""
import os
import re

import numpy as np
import pytest

import bds_amd

import probedata_cases as pc
from test_mex_mock import Mex, MexError, mex  # noqa: F401  (the fixture that builds the gateway against the mock runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["hist_i", "hist_q", "psd", "excerpt_re", "excerpt_im", "stats", "n_segments", "n_samples"]


def test_probe_data_argument_errors(mex):  # noqa: F811
    with pytest.raises(MexError, match=r"probe_data: \(path, settings, signal\[, n_samples\]\)") as e:
        mex.call(1, mex.value("probe_data"), mex.value("x.bin"))
    assert e.value.ident == "bds:args"
    s = bds_amd.init_settings_b2a()
    with pytest.raises(MexError, match=r"settings\.samplingFreq is missing"):
        mex.call(1, mex.value("probe_data"), mex.value("x.bin"), mex.settings(s, drop=("samplingFreq",)), mex.double(2))


def test_wrapper_reads_only_what_the_gateway_returns():
    src = open(os.path.join(ROOT, "mex", "probeData.m")).read()
    assert set(re.findall(r"\bp\.(\w+)", src)) <= set(FIELDS) and "bds_mex('probe_data', fileNameStr, settings, signal)" in src
    assert src.startswith("function probeData(varargin)") and "figure(100)" in src
    gw = open(os.path.join(ROOT, "mex", "bds_mex.c")).read()
    assert [f for f in re.findall(r'out_field\(out, "(\w+)"', gw)] == FIELDS


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["s8", "s8c"])
def test_probe_data_through_the_gateway(mex, tmp_path, fmt):  # noqa: F811
    file_type, data_type = pc.FORMAT_SETTINGS[fmt]
    s = bds_amd.init_settings_b2a(fileType=file_type, dataType=data_type, samplingFreq=8.184e6, skipNumberOfBytes=3)
    cplx = pc.is_complex(fmt)
    n = 5 * 8184  # the reference's window at this rate
    x = pc.quantise(fmt, pc.tone_plus_noise(n + 50, cplx, -2000 if cplx else 2000, 61))
    path = str(tmp_path / "rec.bin")
    pc.encode(fmt, x, lead=3).tofile(path)
    want = bds_amd.probe_data(path, s)
    assert want.n_samples == n
    (out,) = mex.call(1, mex.value("probe_data"), mex.value(path), mex.settings(s), mex.double(2))
    assert mex.fields(out) == FIELDS
    get = lambda f: mex.doubles(mex.L.mxGetField(out, 0, f.encode()))
    assert get("psd").shape == (32768 if cplx else 16385, 1) and np.array_equal(get("psd")[:, 0], want.psd)
    assert get("hist_i").shape == (1, 257) and np.array_equal(get("hist_i")[0], want.hist_i)
    n_time = 4092 if cplx else 16
    assert get("excerpt_re").shape == (1, n_time) and np.array_equal(get("excerpt_re")[0], np.real(want.excerpt))
    if cplx:
        assert np.array_equal(get("hist_q")[0], want.hist_q) and np.array_equal(get("excerpt_im")[0], np.imag(want.excerpt))
    else:
        assert get("hist_q").size == 0 and get("excerpt_im").size == 0
    st = get("stats")[0]
    assert [int(v) for v in st[:4]] == [want.sums[k] for k in ("min_i", "max_i", "sum_i", "sumsq_i")]
    assert int(get("n_segments")[0, 0]) == want.n_segments and int(get("n_samples")[0, 0]) == n
    mex.L.mxDestroyArray(out)
    (out,) = mex.call(1, mex.value("probe_data"), mex.value(path), mex.settings(s), mex.double(2), mex.double(-1))
    assert int(mex.doubles(mex.L.mxGetField(out, 0, b"n_samples"))[0, 0]) == n + 50
    mex.L.mxDestroyArray(out)
    with pytest.raises(MexError, match="Could not read enough data") as e:
        mex.call(1, mex.value("probe_data"), mex.value(path), mex.settings(s), mex.double(2), mex.double(10 ** 6))
    assert e.value.ident == "bds:probe_data"
