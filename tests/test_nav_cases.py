"""Navigation decoding without a GPU: the restatement of tests/nav_cases.py against the reference's own numbers
(tests/golden/nav_tables.json), against deliberately wrong models, and the library's C++ field parser and merger
(bds_nav_fields) bit-equal to the restatement."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest

import nav_cases as nc
from bds_amd import native, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "nav_tables.json")) as _f:
    TABLES = json.load(_f)


def test_restatement_tables_equal_the_reference_literals():
    assert list(nc.FB21) == TABLES["bch21_feedback"] and list(nc.FB51) == TABLES["bch51_feedback"]
    assert TABLES["thresholds"] == {"bch21": nc.THR21, "bch51": nc.THR51, "b2a_sync": nc.THR_SYNC_B2A, "b1c_sync": nc.THR_SYNC_B1C}
    assert list(nc.CRC_EXPONENTS) == TABLES["crc_exponents"]
    assert sum(1 << e for e in nc.CRC_EXPONENTS) == synth.CRC24Q == 0x1864CFB
    assert list(nc.FRAME3_ROWS) == TABLES["frame3_rows"]
    for sig in ("B1C", "B2A"):
        assert sorted(map(tuple, nc.resolved_fields(sig))) == sorted(map(tuple, TABLES["fields"][sig])), sig


def test_builder_layouts_equal_the_reference_ranges():
    """synth.BCNAV1_FIELDS / BCNAV2_FIELDS (what pack_bcnav?_fields write) name the reference's bit ranges."""
    ref = {n: (a, b) for _, n, a, b, *_ in TABLES["fields"]["B1C"]}
    for name, rng_ in synth.BCNAV1_FIELDS.items():
        assert name == "PRN" and rng_ == (1, 6) or ref[name] == rng_, name
    for t, layout in synth.BCNAV2_FIELDS.items():
        ref = {n: (a, b) for g, n, a, b, *_ in TABLES["fields"]["B2A"] if g == str(t)}
        for name, rng_ in layout.items():
            assert ref[name] == rng_, (t, name)
    np.testing.assert_array_equal(synth.BCNAV2_PREAMBLE, nc.ofs.B2A_PREAMBLE_BITS)
    np.testing.assert_array_equal(synth.BCNAV2_SECOND, nc.ofs.B2A_SECOND_CODE)


@pytest.mark.parametrize("k,n,fb,dmin", [(6, 21, nc.FB21, 8), (8, 51, nc.FB51, 24)])
def test_bch_tables_are_systematic_distinct_and_far_apart(k, n, fb, dmin):
    hypo, enc = nc.bch_table(k, n, fb)
    bits = (enc < 0).astype(np.uint8)  # 1 -> -1
    np.testing.assert_array_equal(bits[:, :k], hypo)  # systematic: the first k symbols are the hypothesis
    assert len({tuple(r) for r in bits}) == 1 << k
    d = (bits[:, None, :] != bits[None, :, :]).sum(axis=2)
    assert d[~np.eye(1 << k, dtype=bool)].min() == dmin
    # ... so with the thresholds 20 of 21 / 50 of 51 only an exact code word passes, and the passing maximum is unique
    for h in (0, 1, (1 << k) - 1, 37):
        np.testing.assert_array_equal(synth.bch_codeword(h, k, n, fb), bits[h])


def test_bch_correlations_are_odd():
    """A correlation of two +-1 words of odd length is odd: 20 and 50 are never attained, `maxValue >= threshold` and
    `maxValue > threshold` agree on every input."""
    rng = np.random.default_rng(1)
    for table in (nc._T21, nc._T51):
        x = rng.choice([-1, 1], table[1].shape[1])
        assert np.all((table[1] @ x) % 2 == 1)


def test_crc24q_check_value_and_zero_remainder():
    msg = np.unpackbits(np.frombuffer(b"123456789", dtype=np.uint8))
    c = nc.crc_bits(msg)
    assert int("".join(map(str, c)), 2) == 0xCDE703
    np.testing.assert_array_equal(synth.crc24q(msg), c)
    assert nc.crc_remainder(np.concatenate([msg, c])) == 0
    assert nc.crc_remainder(np.concatenate([msg, c ^ np.eye(24, dtype=np.uint8)[5]])) != 0


def _scaled(raw, a, b, signed, mul, exp, pi):
    w = b - a + 1
    v = raw - (1 << w) if signed and raw >> (w - 1) else raw
    x = float(v) * float(mul) * 2.0 ** exp
    return x * nc.PI if pi else x


def _b1c_series(rng, prn, frames, n):
    """frames: [(index, symbols, sign)] -> (pilot, data) prompt series."""
    pilot = nc.b1c_pilot(rng, n, prn, [i for i, _, _ in frames])
    data = nc.noise_like(rng, n)
    for i, sym, sign in frames:
        nc.place(data, i, sym, rng, sign)
    return pilot, data


@pytest.mark.parametrize("page", [1, 3])
def test_b1c_builder_to_restatement_returns_every_field(page):
    rng = np.random.default_rng(100 + page)
    bits, sym = nc.b1c_message(rng, 19, page)
    pilot, data = _b1c_series(rng, 19, [(37, sym, 1.0)], 1900)
    r = nc.nav_decode_channel("B1C", 19, pilot, data)
    assert len(r["frames"]) == 1 and r["frames"][0]["status"] == nc.BCH1_OK | nc.BCH2_OK | nc.CRC1_OK | nc.CRC2_OK | nc.ENTERED
    np.testing.assert_array_equal(r["frames"][0]["bits"], bits)
    assert r["firstSubFrame"] == 37
    val = lambda a, b: int("".join(map(str, bits[a - 1:b])), 2)  # noqa: E731
    seen = 0
    for g, name, a, b, sg, mul, exp, pi in TABLES["fields"]["B1C"]:
        if g in ("first", "every", f"page{page}") and name not in ("SatType", "PageID"):
            assert r["eph"][name] == _scaled(val(a, b), a, b, sg, mul, exp, pi), name
            seen += 1
    assert seen == 30 + 5 + (18 if page == 1 else 6)
    assert r["eph"]["SatType"] == val(65, 66) or val(65, 66) == 0
    assert r["TOW"] == val(28, 35) * 3600 + val(7, 14) * 18
    other = [n for g, n, *_ in TABLES["fields"]["B1C"] if g == ("page3" if page == 1 else "page1")]
    assert all(math.isnan(r["eph"][n]) for n in other)


@pytest.mark.parametrize("mes_type", [10, 11, 30, 31, 32, 33, 34, 40])
def test_b2a_builder_to_restatement_returns_every_field(mes_type):
    rng = np.random.default_rng(200 + mes_type)
    bits, sym = nc.b2a_message(rng, 27, mes_type)
    ip = nc.noise_like(rng, 3100)
    nc.place(ip, 45, sym, rng)
    r = nc.nav_decode_channel("B2A", 27, ip)
    assert [f["status"] for f in r["frames"]] == [nc.CRC1_OK | nc.ENTERED]
    np.testing.assert_array_equal(r["frames"][0]["bits"], bits)
    val = lambda a, b: int("".join(map(str, bits[a - 1:b])), 2)  # noqa: E731
    group = str(mes_type) if str(mes_type) in nc.B2A_ID_SLOT else "other"
    for g, name, a, b, sg, mul, exp, pi in TABLES["fields"]["B2A"]:
        if g == group and name != "SatType":
            assert r["eph"][name] == _scaled(val(a, b), a, b, sg, mul, exp, pi), name
    assert r["firstSubFrame"] == 45 and r["TOW"] == val(13, 30) * 3 and r["eph"]["PRN"] == 27
    assert list(r["eph"]["idValid"]).count(mes_type) == 1


def _cases_for_models():
    """Prompt-level cases on which every wrong model of nav_cases.Model must differ from the reference's."""
    rng = np.random.default_rng(7)
    cases = []
    b1, s1 = nc.b1c_message(rng, 8, 1, deltaA=(1 << 26) - 5)  # a negative deltaA
    pilot, data = _b1c_series(rng, 8, [(37, s1, 1.0), (1837, s1, -1.0)], 3700)
    cases.append(("B1C", 8, pilot, data))
    flipped = s1.copy()
    flipped[4] = -flipped[4]  # one wrong symbol in 1..21: maxValue 19
    pilot, data = _b1c_series(rng, 8, [(1, flipped, 1.0)], 1800)
    cases.append(("B1C", 8, pilot, data))
    _, s2 = nc.b2a_message(rng, 30, 10, deltaA=(1 << 26) - 5)
    ip = nc.noise_like(rng, 3000)
    nc.place(ip, 1, s2, rng)
    cases.append(("B2A", 30, ip, None))
    return cases


WRONG_MODELS = {
    "rows 2:3:35 for sub-frame 3": nc.Model(frame3_rows=tuple(range(2, 36, 3))),
    "> for >= in the BCH thresholds": nc.Model(bch_ge=False),
    "only the first 21 bits inverted": nc.Model(invert_all=False),
    "CRC over 576 of sub-frame 2's bits": nc.Model(crc2_len=576),
    "> 3000 for >= 3000": nc.Model(short_ge=False),
    "symbol bit taken as > 0": nc.Model(b2a_bit_negative=False),
    "two's complement dropped on deltaA": nc.Model(unsigned_field="deltaA"),
}


def _bch_function_cases():
    """Inputs of the restated BCH21_6Decoding / BCH51_8Decoding themselves, [(table, threshold, bits, hypothesis)]: a code word
    with one symbol erased.  Both functions take any real row vector (`sum(encoded .* bits)`, BCH21_6Decoding.m:91), and an erased
    symbol, 0, leaves maxValue at exactly 20 / 50: the one place where `>=` (:97 / BCH51_8Decoding.m:95) and `>` part.  No series
    of prompts gets there -- BCNAV1decoding.m hands over +-1, whose correlations over 21 or 51 symbols are odd
    (test_bch_correlations_are_odd) -- so the comparison is held at the functions."""
    cases = []
    for table, thr, h, erased in ((nc._T21, nc.THR21, 37, 9), (nc._T51, nc.THR51, 200, 30), (nc._T21, nc.THR21, 0, 0)):
        x = table[1][h].astype(np.float64)
        x[erased] = 0.0
        cases.append((table, thr, x, h))
    return cases


def test_bch_functions_accept_a_maximum_equal_to_the_threshold():
    for table, thr, x, h in _bch_function_cases():
        ok, bits, mx = nc.bch_decode(x, table, thr)
        assert ok and mx == thr and int("".join(map(str, bits)), 2) == h
        ok, _, mx = nc.bch_decode(-x, table, thr)  # the other polarity: nowhere near
        assert not ok and mx < thr


@pytest.mark.parametrize("what", list(WRONG_MODELS))
def test_the_cases_reject_a_wrong_model(what):
    """Each deliberately changed model must give another result than the reference's on at least one case: the prompt-level
    cases through the whole decoding loop, and the BCH functions' own cases (_bch_function_cases), which alone can tell `>`
    from `>=` in their thresholds."""
    model = WRONG_MODELS[what]
    differs = False
    for sig, prn, sync, data in _cases_for_models():
        a = nc.nav_decode_channel(sig, prn, sync, data)
        b = nc.nav_decode_channel(sig, prn, sync, data, model=model)
        if nc.same_frames(a["frames"], b["frames"]) or nc.same_eph(a["eph"], b["eph"]) or a["TOW"] != b["TOW"]:
            differs = True
    for table, thr, x, _ in _bch_function_cases():
        a = nc.bch_decode(x, table, thr, nc.REFERENCE.bch_ge)
        b = nc.bch_decode(x, table, thr, model.bch_ge)
        if a[0] != b[0]:
            differs = True
    assert differs, what


# ---- the library's parser and merger -----------------------------------------------------------------------------------------------
def test_header_struct_and_binding_agree():
    src = open(os.path.join(ROOT, "include", "bds_mi355x.h")).read()
    body = re.search(r"#define BDS_EPH_FIELDS\(X\)(.*?)\ntypedef struct bds_eph", src, re.S).group(1)
    assert re.findall(r"X\((\w+)\)", body) == native.EPH_FIELDS == nc.EPH_FIELDS
    assert ctypes.sizeof(native.Eph) == 4 * 4 + 8 * 4 + 8 * len(native.EPH_FIELDS)
    assert ctypes.sizeof(native.NavFrame) == 24 + 112
    for entry in ("bds_nav_decode", "bds_nav_fields"):
        assert re.search(r"BDS_API\s+int\s+%s\s*\(" % entry, src) and entry in native.EXPORTS and hasattr(native.lib(), entry)
    e = native.Eph()  # .size not set: refused
    assert native.lib().bds_nav_fields(1, None, 0, 110, ctypes.byref(e)) == -1


def _random_message(rng, sig, kind):
    n = 878 if sig == "B1C" else 288
    m = rng.integers(0, 2, n).astype(np.uint8)
    prn = int(rng.integers(1, 64))
    m[:6] = [(prn >> (5 - i)) & 1 for i in range(6)]
    at = 614 if sig == "B1C" else 6  # PageID / MesType
    m[at:at + 6] = [(kind >> (5 - i)) & 1 for i in range(6)]
    return m


@pytest.mark.parametrize("sig,kind", [("B1C", 1), ("B1C", 3), ("B1C", 2)] + [("B2A", t) for t in (10, 11, 30, 31, 32, 33, 34, 5)])
def test_library_parser_is_bit_equal_to_the_restatement(sig, kind):
    rng = np.random.default_rng(1000 + kind)
    for _ in range(200):
        m = _random_message(rng, sig, kind)
        got, n = native.nav_fields(sig, m)
        want, n_ref = nc.nav_fields_ref(sig, [m])
        assert n == n_ref == 1 and nc.same_eph(got, want) is None, nc.same_eph(got, want)


@pytest.mark.parametrize("sig", ["B1C", "B2A"])
def test_library_merger_is_bit_equal_to_the_restatement(sig):
    """Sequences of messages: first-frame gates, later pages / types, PRN fields 0 in between (not entered), all ones, all zeros."""
    rng = np.random.default_rng(5)
    kinds = [1, 3, 2, 1] if sig == "B1C" else [10, 11, 30, 31, 32, 33, 34, 17]
    n = 878 if sig == "B1C" else 288
    for trial in range(60):
        seq = [_random_message(rng, sig, int(rng.choice(kinds))) for _ in range(int(rng.integers(1, 6)))]
        if trial % 3 == 0:
            seq[int(rng.integers(0, len(seq)))][:6] = 0  # PRN field 0
        if trial % 7 == 0:
            seq.insert(int(rng.integers(0, len(seq) + 1)), np.ones(n, dtype=np.uint8))  # PRN 63
        if trial % 11 == 0:
            seq.insert(0, np.zeros(n, dtype=np.uint8))
        got, k = native.nav_fields(sig, np.stack(seq))
        want, k_ref = nc.nav_fields_ref(sig, seq)
        assert k == k_ref and nc.same_eph(got, want) is None, (trial, nc.same_eph(got, want))
    got, k = native.nav_fields(sig, np.zeros((2, n), dtype=np.uint8))
    assert k == 0 and got["flag"] == 0 and all(math.isnan(got[f]) for f in native.EPH_FIELDS)
