"""bds_mex('blank_pulses', ...) EXECUTED against the stand-in for the MEX runtime (tests/mex_stub, as tests/test_probedata_mex.py
does for 'probe_data'): argument checks, the fields mex/blankPulses.m reads, and file and report against the NumPy model.
mex/blankPulses.m itself needs MATLAB to run; here it is held to the fields the gateway returns."""
import os
import re

import numpy as np
import pytest

import blank_cases as bc
from test_mex_mock import Mex, MexError, mex  # noqa: F401  (the fixture that builds the gateway against the mock runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["n_samples", "n_flagged", "n_blanked", "n_runs", "threshold_sq", "duty"]
USAGE = r"blank_pulses: \(path_in, path_out, settings, signal, threshold, pre, post\[, duty_samples\[, piece_samples\]\]\)"


def test_blank_pulses_argument_errors(mex, tmp_path):  # noqa: F811
    with pytest.raises(MexError, match=USAGE) as e:
        mex.call(1, mex.value("blank_pulses"), mex.value("a.bin"), mex.value("b.bin"))
    assert e.value.ident == "bds:args"
    s = bc.settings_of("s8")
    args = lambda **kw: (mex.value("blank_pulses"), mex.value(kw.get("src", "a.bin")), mex.value(str(tmp_path / "never.bin")), mex.settings(s, drop=kw.get("drop", ())),
                         mex.double(2), mex.double(kw.get("thr", 100.0)), mex.double(25), mex.double(25), mex.double(kw.get("ds", 0)))
    with pytest.raises(MexError, match=r"settings\.samplingFreq is missing"):
        mex.call(1, *args(drop=("samplingFreq",)))
    with pytest.raises(MexError, match="threshold must be an amplitude") as e:
        mex.call(1, *args(thr=-1.0))
    assert e.value.ident == "bds:args"
    with pytest.raises(MexError, match="Unable to read file") as e:
        mex.call(1, *args(src=str(tmp_path / "missing.bin"), ds=100))
    assert e.value.ident == "bds:blank_pulses" and not os.path.exists(tmp_path / "never.bin")


def test_wrapper_reads_only_what_the_gateway_returns():
    src = open(os.path.join(ROOT, "mex", "blankPulses.m")).read()
    assert set(re.findall(r"\breport\.(\w+)", src)) <= set(FIELDS)
    assert "bds_mex('blank_pulses', fileIn, fileOut, settings, signal, threshold, pre, post, dutySamples)" in src
    assert src.startswith("function report = blankPulses(fileIn, fileOut, settings, threshold, pre, post, dutySamples)")
    gw = open(os.path.join(ROOT, "mex", "bds_mex.c")).read()
    assert re.findall(r'out_field\(rep, "(\w+)"', gw) == FIELDS


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["s8", "s8c"])
def test_blank_pulses_through_the_gateway(mex, tmp_path, fmt):  # noqa: F811
    _, _, dt, c = bc.FORMATS[fmt]
    skip, n = 3, bc.T + 501
    s = bc.settings_of(fmt, skipNumberOfBytes=skip)
    rec = bc.with_hits(fmt, n, [0, 700, 730, bc.T - 1, bc.T, n - 1], seed=11)
    header = (np.arange(skip * c) + 5).astype(dt)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([header, rec]).tofile(src)
    want, wrep = bc.model(rec, fmt, 2500, 25, 30, duty_samples=1000)
    (out,) = mex.call(1, mex.value("blank_pulses"), mex.value(src), mex.value(dst), mex.settings(s), mex.double(2), mex.double(50.5), mex.double(25),
                      mex.double(30), mex.double(1000), mex.double(600))
    assert mex.fields(out) == FIELDS
    get = lambda f: mex.doubles(mex.L.mxGetField(out, 0, f.encode()))
    assert [int(get(f)[0, 0]) for f in FIELDS[:5]] == [n, wrep["n_flagged"], wrep["n_blanked"], wrep["n_runs"], 2550]
    assert get("duty").shape == (wrep["duty"].size, 1) and np.array_equal(get("duty")[:, 0], wrep["duty"])
    mex.L.mxDestroyArray(out)
    back = np.fromfile(dst, dtype=dt)
    assert np.array_equal(back[:skip * c], header) and np.array_equal(back[skip * c:], bc.model(rec, fmt, 2550, 25, 30)[0])
    (out,) = mex.call(1, mex.value("blank_pulses"), mex.value(src), mex.value(dst), mex.settings(s), mex.double(2), mex.double(50.0), mex.double(25), mex.double(30))
    assert get("duty").size == 0 and int(get("n_blanked")[0, 0]) == wrep["n_blanked"]
    mex.L.mxDestroyArray(out)
    with pytest.raises(MexError, match="too small for its context") as e:
        mex.call(1, mex.value("blank_pulses"), mex.value(src), mex.value(dst), mex.settings(s), mex.double(2), mex.double(50.0), mex.double(25), mex.double(30),
                 mex.double(0), mex.double(30))
    assert e.value.ident == "bds:blank_pulses"
