"""bds_mex('corr_function', ...) EXECUTED against the stand-in for the MEX runtime (tests/mex_stub, as tests/test_probedata_mex.py
does for probe_data): argument errors, the field names, I and Q against Context.corr_function on the same file.
mex/corrFunction.m itself needs MATLAB to run; here it is held to the fields the gateway returns."""
import os
import re

import numpy as np
import pytest

import bds_amd

import corrfn_cases as cc
from test_mex_mock import Mex, MexError, mex  # noqa: F401  (the fixture that builds the gateway against the mock runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["I", "Q", "n_comp"]


def test_corr_function_argument_errors(mex):  # noqa: F811
    s = bds_amd.init_settings_b2a()
    st = np.zeros(6)
    with pytest.raises(MexError, match=r"corr_function: \(path, settings, prn, state6, taps\)") as e:
        mex.call(1, mex.value("corr_function"), mex.value("x.bin"), mex.settings(s), mex.double(19))
    assert e.value.ident == "bds:args"
    with pytest.raises(MexError, match=r"settings\.samplingFreq is missing"):
        mex.call(1, mex.value("corr_function"), mex.value("x.bin"), mex.settings(s, drop=("samplingFreq",)), mex.double(19), mex.double(st),
                 mex.double(0.0))
    with pytest.raises(MexError, match=r"state6 must be 6 x numel\(prn\)"):
        mex.call(1, mex.value("corr_function"), mex.value("x.bin"), mex.settings(s), mex.double([19, 20]), mex.double(st), mex.double(0.0))
    with pytest.raises(MexError, match=r"1 \.\. 128 taps"):
        mex.call(1, mex.value("corr_function"), mex.value("x.bin"), mex.settings(s), mex.double(19), mex.double(st), mex.double(np.zeros(129)))


def test_wrapper_reads_only_what_the_gateway_returns():
    src = open(os.path.join(ROOT, "mex", "corrFunction.m")).read()
    assert set(re.findall(r"\bp\.(\w+)", src)) <= set(FIELDS)
    assert "bds_mex('corr_function', fileNameStr, settings, prn, state6, taps(:).')" in src
    assert src.startswith("function [R, taps] = corrFunction(fileNameStr, trackResults, channel, settings, taps, epochs)") and "figure(300)" in src
    # the states as bds_amd.track_states builds them: the epoch's own entries, blksize from them
    for text in ("r.absoluteSample(e); blksize; r.remCodePhase(e); r.codeFreq(e); r.remCarrPhase(e); r.carrFreq(e)",
                 "ceil((settings.codeLength - r.remCodePhase(e)) / step)", "step = r.codeFreq(e) / settings.samplingFreq"):
        assert text in src, text
    gw = open(os.path.join(ROOT, "mex", "bds_mex.c")).read()
    body = gw[gw.index("static void do_corr_function"):gw.index("void mexFunction")]
    assert re.findall(r'out_field\(res, "(\w+)"', body) + re.findall(r'mxAddField\(res, "(\w+)"', body) == FIELDS


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["B2A", "WB"])
def test_corr_function_through_the_gateway(ctx, mex, tmp_path, mode):  # noqa: F811
    signal = "B2A" if mode == "B2A" else "B1C"
    s, x, chans, trace, _ = cc.traced(signal, mode, 3)
    prn, st = cc.states_of([t for t in trace if t["k"] in (1, 3)], chans)
    taps = cc.gpu_taps(s.dllCorrelatorSpacing)[2:11]
    path = str(tmp_path / "rec.bin")
    x.tofile(path)
    want = ctx.corr_function(s, path, prn, st, taps)
    (out,) = mex.call(1, mex.value("corr_function"), mex.value(path), mex.settings(s), mex.double(prn), mex.double(st.reshape(-1)),
                      mex.double(taps))
    assert mex.fields(out) == FIELDS
    get = lambda f: mex.doubles(mex.L.mxGetField(out, 0, f.encode()))
    n_comp = int(get("n_comp")[0, 0])
    assert n_comp == want.shape[1] == (2 if mode == "B2A" else 3)
    I, Q = get("I"), get("Q")
    assert I.shape == Q.shape == (len(taps) * n_comp, len(prn))
    got = (I + 1j * Q).T.reshape(len(prn), n_comp, len(taps))  # column k: item k, tap fastest, then component
    np.testing.assert_array_equal(got, want)
    mex.L.mxDestroyArray(out)
    bad = st.copy()
    bad[-1, 1] = x.size  # past the end of the record
    with pytest.raises(MexError, match="reaches past the end of the record") as e:
        mex.call(1, mex.value("corr_function"), mex.value(path), mex.settings(s), mex.double(prn), mex.double(bad.reshape(-1)), mex.double(taps))
    assert e.value.ident == "bds:corr_function"
