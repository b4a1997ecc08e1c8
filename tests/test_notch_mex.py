"""bds_mex('notch_tones', ...) EXECUTED against the stand-in for the MEX runtime (tests/mex_stub, as tests/test_blank_mex.py does
for 'blank_pulses'): argument checks, the fields mex/notchTones.m reads, and file, report and estimates against the NumPy model.
mex/notchTones.m itself needs MATLAB to run; here it is held to the fields the gateway returns."""
import os
import re

import numpy as np
import pytest

import notch_cases as nc
from test_mex_mock import Mex, MexError, mex  # noqa: F401  (the fixture that builds the gateway against the mock runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["n_samples", "n_blocks", "n_saturated", "sum_sq_in", "sum_sq_out", "steps", "est_re", "est_im"]
USAGE = r"notch_tones: \(path_in, path_out, settings, signal, freqs, block_log2\[, piece_samples\]\)"


def test_notch_tones_argument_errors(mex, tmp_path):  # noqa: F811
    with pytest.raises(MexError, match=USAGE) as e:
        mex.call(1, mex.value("notch_tones"), mex.value("a.bin"), mex.value("b.bin"))
    assert e.value.ident == "bds:args"
    s = nc.settings_of("s8")
    args = lambda **kw: (mex.value("notch_tones"), mex.value(kw.get("src", "a.bin")), mex.value(str(tmp_path / "never.bin")), mex.settings(s, drop=kw.get("drop", ())),
                         mex.double(2), mex.double(kw.get("freqs", [6.9e6])), mex.double(kw.get("beta", 10)))
    with pytest.raises(MexError, match=r"settings\.samplingFreq is missing"):
        mex.call(1, *args(drop=("samplingFreq",)))
    with pytest.raises(MexError, match="freqs holds 1 to 8 frequencies") as e:
        mex.call(1, *args(freqs=[1e6 * k for k in range(1, 10)]))
    assert e.value.ident == "bds:args"
    with pytest.raises(MexError, match="block_log2 runs from 8 to 16") as e:
        mex.call(1, *args(beta=7))
    assert e.value.ident == "bds:args"
    with pytest.raises(MexError, match="Unable to read file") as e:
        mex.call(1, *args(src=str(tmp_path / "missing.bin")))
    assert e.value.ident == "bds:notch_tones" and not os.path.exists(tmp_path / "never.bin")


def test_wrapper_reads_only_what_the_gateway_returns():
    src = open(os.path.join(ROOT, "mex", "notchTones.m")).read()
    assert set(re.findall(r"\breport\.(\w+)", src)) <= set(FIELDS)
    assert "bds_mex('notch_tones', fileIn, fileOut, settings, signal, double(freqs(:).'), blockLog2)" in src
    assert src.startswith("function report = notchTones(fileIn, fileOut, settings, freqs, blockLog2)")
    gw = open(os.path.join(ROOT, "mex", "bds_mex.c")).read()
    assert re.findall(r'out_field\(nr, "(\w+)"', gw) == FIELDS


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["s8", "s8c"])
def test_notch_tones_through_the_gateway(mex, tmp_path, fmt):  # noqa: F811
    _, _, dt, c = nc.FORMATS[fmt]
    skip, n, beta = 3, 5 * 256 + 37, 8
    fs = 25e6
    s = nc.settings_of(fmt, skipNumberOfBytes=skip, samplingFreq=fs)
    freqs = [6.9e6, 2.2e6 + 0.3] if fmt == "s8" else [-3.3e6, 1.7e6 + 0.3]
    steps = [int(np.floor(f / fs * 2 ** 32 + 0.5)) % 2 ** 32 for f in freqs]
    rec = nc.with_tones(fmt, n, steps, seed=12)
    header = (np.arange(skip * c) + 5).astype(dt)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([header, rec]).tofile(src)
    want, wrep = nc.model(rec, fmt, steps, beta)
    for extra in ((), (mex.double(512),)):
        (out,) = mex.call(1, mex.value("notch_tones"), mex.value(src), mex.value(dst), mex.settings(s), mex.double(2), mex.double(freqs), mex.double(beta), *extra)
        assert mex.fields(out) == FIELDS
        get = lambda f: mex.doubles(mex.L.mxGetField(out, 0, f.encode()))
        assert [int(get(f)[0, 0]) for f in FIELDS[:5]] == [n, wrep["n_blocks"], wrep["n_saturated"], wrep["sum_sq_in"], wrep["sum_sq_out"]]
        assert get("steps").shape == (1, 2) and [int(v) for v in get("steps")[0]] == steps
        assert get("est_re").shape == (wrep["n_blocks"], 2)
        assert np.array_equal(get("est_re") * 256, wrep["est"][..., 0]) and np.array_equal(get("est_im") * 256, wrep["est"][..., 1])
        mex.L.mxDestroyArray(out)
        back = np.fromfile(dst, dtype=dt)
        assert np.array_equal(back[:skip * c], header) and np.array_equal(back[skip * c:], want)
    with pytest.raises(MexError, match="smaller than one block") as e:
        mex.call(1, mex.value("notch_tones"), mex.value(src), mex.value(dst), mex.settings(s), mex.double(2), mex.double(freqs), mex.double(beta), mex.double(100))
    assert e.value.ident == "bds:notch_tones"
