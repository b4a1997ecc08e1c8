"""Navigation decoding: a float64 / NumPy restatement of the reference's decoders, field parsers and merging loops, and the
builder of the prompt-level cases the tests feed to bds_nav_decode.  Test infrastructure only; nothing here is loaded by the
library.

Restated, with the reference's line numbers:
    B1C/include/BCNAV1decoding.m:100-189, BCH21_6Decoding.m:49-103, BCH51_8Decoding.m:47-101, B1C/include/ephemeris.m:66-237
    B2a/include/BCNAV2decoding.m:103-159, B2a/include/ephemeris.m:60-310, Common/twosComp2dec.m:39-44
The frame-sync half (the `index` lists) is oracle/framesync.py.

`Model` holds the choices at which a restatement can silently go wrong; the defaults are the reference's, and
tests/test_nav_cases.py shows that each other setting is caught: by the builder's prompt-level cases, and `bch_ge` -- which no
series of +-1 prompts can reach -- by inputs of the BCH functions themselves.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from oracle import codes as ocodes
from oracle import framesync as ofs

PI = 3.1415926535898  # bdsPi / gpsPi
FB21, FB51 = (2, 4, 5, 6), (1, 4, 5, 6, 7, 8)  # BCH21_6Decoding.m:62, BCH51_8Decoding.m:60
THR21, THR51 = 20, 50  # :49 / :47
THR_SYNC_B1C, THR_SYNC_B2A = 1799.5, 115  # BCNAV1decoding.m:91, BCNAV2decoding.m:97
CRC_EXPONENTS = (24, 23, 18, 17, 14, 11, 10, 7, 6, 5, 4, 3, 1, 0)  # comm.CRCDetector(...), BCNAV1decoding.m:97
FRAME3_ROWS = tuple(range(3, 36, 3))  # Frame3Colum = 3:3:35 (:147), 1-based rows of the 36 x 48 block

# status flags, polarity and maxima as include/bds_mi355x.h defines them
SHORT, BCH1_OK, BCH2_OK, CRC1_OK, CRC2_OK, ENTERED, PRN_RANGE = 1, 2, 4, 8, 16, 32, 64

EPH_FIELDS = ["PRN", "SOH", "SOW", "WN", "HOW", "IODC", "IODE", "IODC_MSB2", "IODC_LSB8",
              "t_oe", "deltaA", "ADot", "delta_n_0", "delta_n_0Dot", "M_0", "e", "omega",
              "omega_0", "i_0", "omegaDot", "i_0Dot", "C_is", "C_ic", "C_rs", "C_rc", "C_us", "C_uc",
              "t_oc", "a_0", "a_1", "a_2", "T_GDB2ap", "ISC_B1Cd", "T_GDB1Cp",
              "PageID1", "PageID3", "HS", "DIF", "SIF", "AIF", "SISMAI",
              "alpha1", "alpha2", "alpha3", "alpha4", "alpha5", "alpha6", "alpha7", "alpha8", "alpha9",
              "A_0UTC", "A_1UTC", "A_2UTC", "delta_t_LS", "t_ot", "WN_ot", "WN_LSF", "DN", "delta_t_LSF",
              "GNSS_ID", "WN_0BGTO", "t_0BGTO", "A_0BGTO", "A_1BGTO", "A_2BGTO", "TOW"]


@dataclass(frozen=True)
class Model:
    frame3_rows: tuple = FRAME3_ROWS  # rows of sub-frame 3
    bch_ge: bool = True               # maxValue >= threshold (else >)
    invert_all: bool = True           # bits = 1 - bits over all 1800 (else over the first 21 only)
    crc2_len: int = 600               # bits of sub-frame 2 under its CRC
    short_ge: bool = True             # length - index + 1 >= 3000 (else >)
    b2a_bit_negative: bool = True     # NavDataLogic = navBits < 0.5 (else > 0)
    unsigned_field: str = ""          # a signed field read with bin2dec instead of twosComp2dec


REFERENCE = Model()


# ---- code tables and CRC -------------------------------------------------------------------------------------------------------
def bch_table(k, n, feedback):
    """(hypoBits [2^k, k] of 0 / 1, encoded [2^k, n] of +-1) -- the hypothesis loop of BCH21_6Decoding.m:65-92."""
    hypo = np.zeros((1 << k, k), dtype=np.int64)
    enc = np.zeros((1 << k, n), dtype=np.int64)
    for h in range(1 << k):
        digits = [int(c) for c in format(h, "b").zfill(k)]  # dec2bin, padded on the left (:68-69)
        hypo[h] = digits
        reg = [1 if d == 0 else -1 for d in digits][::-1]  # 0 -> 1, 1 -> -1, then fliplr (:75-79)
        for s in range(n):
            enc[h, s] = reg[-1]
            fbk = int(np.prod([reg[p - 1] for p in feedback]))
            reg = [fbk] + reg[:-1]  # circshift by one, then register1(1) = feedback1 (:87-88)
    return hypo, enc


_T21 = bch_table(6, 21, FB21)
_T51 = bch_table(8, 51, FB51)


def bch_decode(check, table, threshold, ge=True):
    """[flag, decodedBits, maxValue] of BCH21_6Decoding.m:91-103 on `check`: +-1 from the decoding loop, any real row vector
    as far as the function goes."""
    hypo, enc = table
    corr = enc @ np.asarray(check, dtype=np.float64)
    pos = int(np.argmax(corr))  # MATLAB's max: the first of equal maxima
    mx = corr[pos]
    ok = mx >= threshold if ge else mx > threshold
    return ok, hypo[pos].copy(), mx


def crc_remainder(bits):
    """Remainder (int, 24 bits) of the 0 / 1 sequence `bits`, first bit = highest power, divided by the generator given by
    CRC_EXPONENTS; zero initial state, nothing reflected or inverted.  comm.CRCDetector with its default properties reports no
    error exactly when message + checksum leave remainder 0."""
    poly = sum(1 << e for e in CRC_EXPONENTS)
    r = 0
    for b in np.asarray(bits).astype(int).tolist():
        r = (r << 1) | b
        if r >> 24:
            r ^= poly
    return r


def crc_bits(bits):
    """The 24 checksum bits to append to `bits`."""
    r = crc_remainder(list(np.asarray(bits).astype(int)) + [0] * 24)
    return np.array([(r >> (23 - i)) & 1 for i in range(24)], dtype=np.uint8)


# ---- the frame decoders ----------------------------------------------------------------------------------------------------------
def _frame(index):
    return {"index": int(index), "status": 0, "polarity": 0, "bch1_max": 0, "bch2_max": 0}


def decode_b1c_frame(i_p, index, model=REFERENCE):
    """One pass of the loop body BCNAV1decoding.m:104-173 for index(i) = `index` (1-based)."""
    f = _frame(index)
    f["bits"] = np.zeros(878, dtype=np.uint8)
    x = np.asarray(i_p, dtype=np.float64)[index - 1:index - 1 + 1800]
    assert x.size == 1800
    bits = np.where(x > 0, 1, 0).astype(np.int64)  # :105-106 (NaN > 0 is false)
    ok, dec1, mx = bch_decode(1 - 2 * bits[:21], _T21, THR21, model.bch_ge)  # :110-112
    pol = 1
    if not ok:  # :116-126
        if model.invert_all:
            bits = 1 - bits
        else:
            bits = np.concatenate([1 - bits[:21], bits[21:]])
        ok, dec1, mx = bch_decode(1 - 2 * bits[:21], _T21, THR21, model.bch_ge)
        pol = -1
    f["bch1_max"] = int(mx)
    if not ok:
        return f
    f["status"] |= BCH1_OK
    f["polarity"] = pol
    ok, dec2, mx2 = bch_decode(1 - 2 * bits[21:72], _T51, THR51, model.bch_ge)  # :133-135
    f["bch2_max"] = int(mx2)
    if not ok:
        return f
    f["status"] |= BCH2_OK
    temp = bits[72:].reshape((36, 48), order="F")  # :146
    rows3 = [r - 1 for r in model.frame3_rows]
    rows2 = [r for r in range(36) if r not in rows3]  # setdiff(1:36, Frame3Colum), :148
    frame2 = temp[rows2, :].reshape(-1)  # reshape(Frame2', 1, 1200): row after row (:150-151)
    frame3 = temp[rows3, :].reshape(-1)  # :153-154
    nav = np.concatenate([dec1, dec2, frame2[:600], frame3[:264]]).astype(np.uint8)  # :129,142,161,163
    f["bits"] = nav
    if crc_remainder(frame2[:model.crc2_len]) == 0:  # :167-168
        f["status"] |= CRC1_OK
    if crc_remainder(frame3[:264]) == 0:  # :171-172
        f["status"] |= CRC2_OK
    return f


def decode_b2a_frame(i_p, index, model=REFERENCE):
    """The loop body BCNAV2decoding.m:105-138."""
    f = _frame(index)
    f["bits"] = np.zeros(288, dtype=np.uint8)
    bits = ofs.threshold_bits(i_p)  # :86-87
    room = bits.size - index + 1
    if not (room >= 3000 if model.short_ge else room > 3000):  # :105
        f["status"] = SHORT
        return f
    temp = bits[index - 1:index - 1 + 3000]
    sym = (temp.reshape(600, 5) * ofs.B2A_SECOND_CODE).sum(axis=1)  # :112-115
    sym = np.where(sym > 0, 1.0, -1.0)  # :118-119
    pol = 1
    if not np.array_equal(sym[:24], ofs.B2A_PREAMBLE_BITS):  # :122-124
        sym = -sym
        pol = -1
    dec = sym[24:][:288]  # :127,132
    logic = dec < 0.5 if model.b2a_bit_negative else dec > 0  # :136
    f["polarity"] = pol
    f["bits"] = logic.astype(np.uint8)
    if crc_remainder(logic) == 0:  # :138
        f["status"] |= CRC1_OK
    return f


# ---- field parsers ---------------------------------------------------------------------------------------------------------------
# (name, first, last, signed, mul, exp, pi): value = int(bits first..last of the block) * mul * 2^exp [* pi]; of mul and
# 2^exp at most one differs from 1, so the product is the reference's single multiplication.  Ranges are relative to the
# block named in front, exactly as the reference slices (subFra2Bit / tempBit); B1C_BLOCKS / B2A_FIELDS resolve them.
def _u(name, a, b, mul=1, exp=0): return (name, a, b, False, mul, exp, False)  # noqa: E704
def _s(name, a, b, exp=0, pi=False): return (name, a, b, True, 1, exp, pi)  # noqa: E704


B1C_BLOCKS = [  # (group, first bit of the block in navBitsBin, fields)
    ("first", 1, [_u("SOH", 7, 14, mul=18)]),  # ephemeris.m:74
    ("first", 15, [_u("WN", 1, 13), _u("HOW", 14, 21), _u("IODC", 22, 32), _u("IODE", 32, 39)]),  # :77-85 (32 twice, as there)
    ("first", 54, [_u("t_oe", 1, 11, mul=300), _u("SatType", 12, 13), _s("deltaA", 14, 39, -9), _s("ADot", 40, 64, -21),
                   _s("delta_n_0", 65, 81, -44, True), _s("delta_n_0Dot", 82, 104, -57, True), _s("M_0", 105, 137, -32, True),
                   _u("e", 138, 170, exp=-34), _s("omega", 171, 203, -32, True)]),  # :88-113
    ("first", 257, [_s("omega_0", 1, 33, -32, True), _s("i_0", 34, 66, -32, True), _s("omegaDot", 67, 85, -44, True),
                    _s("i_0Dot", 86, 100, -44, True), _s("C_is", 101, 116, -30), _s("C_ic", 117, 132, -30),
                    _s("C_rs", 133, 156, -8), _s("C_rc", 157, 180, -8), _s("C_us", 181, 201, -30),
                    _s("C_uc", 202, 222, -30)]),  # :116-140
    ("first", 479, [_u("t_oc", 1, 11, mul=300), _s("a_0", 12, 36, -34), _s("a_1", 37, 58, -50), _s("a_2", 59, 69, -66)]),  # :143-151
    ("first", 548, [_s("T_GDB2ap", 1, 12, -34), _s("ISC_B1Cd", 13, 24, -34), _s("T_GDB1Cp", 25, 36, -34)]),  # :154-160
    ("every", 615, [_u("PageID", 1, 6), _u("HS", 7, 8), _u("DIF", 9, 9), _u("SIF", 10, 10), _u("AIF", 11, 11),
                    _u("SISMAI", 12, 15)]),  # :164-176
    ("page1", 615 + 43 - 1, [_u("alpha1", 1, 10, exp=-3), _s("alpha2", 11, 18, -3), _u("alpha3", 19, 26, exp=-3),
                             _u("alpha4", 27, 34, exp=-3), _u("alpha5", 35, 42, exp=-3), _s("alpha6", 43, 50, -3),
                             _s("alpha7", 51, 58, -3), _s("alpha8", 59, 66, -3), _s("alpha9", 67, 74, -3)]),  # :182-191
    ("page1", 615 + 117 - 1, [_s("A_0UTC", 1, 16, -35), _s("A_1UTC", 17, 29, -51), _s("A_2UTC", 30, 36, -68),
                              _s("delta_t_LS", 37, 44), _u("t_ot", 45, 60, exp=4), _u("WN_ot", 61, 73), _u("WN_LSF", 74, 86),
                              _u("DN", 87, 89), _s("delta_t_LSF", 90, 97)]),  # :194-212
    ("page3", 615 + 159 - 1, [_u("GNSS_ID", 1, 3), _u("WN_0BGTO", 4, 16), _u("t_0BGTO", 17, 32, exp=4), _s("A_0BGTO", 33, 48, -35),
                              _s("A_1BGTO", 49, 61, -51), _s("A_2BGTO", 62, 68, -68)]),  # :217-229
]
_B2A_SOW = _u("SOW", 13, 30, mul=3)
_B2A_CLOCK = [_u("t_oc", 43, 53, mul=300), _s("a_0", 54, 78, -34), _s("a_1", 79, 100, -50), _s("a_2", 101, 111, -66),
              _u("IODC_MSB2", 112, 113), _u("IODC_LSB8", 114, 121)]
B2A_FIELDS = {  # by message type, in the reference's order of assignment (B2a/include/ephemeris.m)
    "10": [_B2A_SOW, _u("WN", 31, 43), _u("DIF", 44, 44), _u("SIF", 45, 45), _u("AIF", 46, 46), _u("t_oe", 62, 72, mul=300),
           _u("SatType", 73, 74), _s("deltaA", 75, 100, -9), _s("ADot", 101, 125, -21), _s("delta_n_0", 126, 142, -44, True),
           _s("delta_n_0Dot", 143, 165, -57, True), _s("M_0", 166, 198, -32, True), _u("e", 199, 231, exp=-34),
           _s("omega", 232, 264, -32, True)],  # :76-117
    "11": [_B2A_SOW, _u("HS", 31, 32), _u("DIF", 33, 33), _u("SIF", 34, 34), _u("AIF", 36, 36),  # (36, not 35: :135)
           _s("omega_0", 43, 75, -32, True), _s("i_0", 76, 108, -32, True), _s("omegaDot", 109, 127, -44, True),
           _s("i_0Dot", 128, 142, -44, True), _s("C_is", 143, 158, -30), _s("C_ic", 159, 174, -30), _s("C_rs", 175, 198, -8),
           _s("C_rc", 199, 222, -8), _s("C_us", 223, 243, -30), _s("C_uc", 244, 264, -30)],  # :119-155
    "30": [_B2A_SOW] + _B2A_CLOCK + [_u("alpha1", 146, 155, exp=-3), _s("alpha2", 156, 163, -3), _u("alpha3", 164, 171, exp=-3),
                                     _u("alpha4", 172, 179, exp=-3), _u("alpha5", 180, 187, exp=-3), _s("alpha6", 188, 195, -3),
                                     _s("alpha7", 196, 203, -3), _s("alpha8", 204, 211, -3), _s("alpha9", 212, 219, -3)],  # :157-187
    "31": [_B2A_SOW] + _B2A_CLOCK,  # :189-210
    "32": [_B2A_SOW] + _B2A_CLOCK,  # :212-233
    "33": [_B2A_SOW] + _B2A_CLOCK + [_u("GNSS_ID", 112, 114), _u("WN_0BGTO", 115, 127), _u("t_0BGTO", 128, 143, exp=4),
                                     _s("A_0BGTO", 144, 159, -35), _s("A_1BGTO", 160, 172, -51), _s("A_2BGTO", 173, 179, -68)],  # :235-263
    "34": [_B2A_SOW, _u("t_oc", 65, 75, mul=300), _s("a_0", 76, 100, -34), _s("a_1", 101, 122, -50), _s("a_2", 123, 133, -66),
           _u("IODC_MSB2", 134, 135), _u("IODC_LSB8", 136, 143),
           # :288-296: nine fields, one bit range
           _s("A_0UTC", 123, 133, -35), _s("A_1UTC", 123, 133, -51), _s("A_2UTC", 123, 133, -68), _s("delta_t_LS", 123, 133),
           _u("t_ot", 123, 133, exp=4), _u("WN_ot", 123, 133), _u("WN_LSF", 123, 133), _u("DN", 123, 133),
           _s("delta_t_LSF", 123, 133)],  # :266-296
    "other": [_B2A_SOW],  # :299-308
}
B2A_ID_SLOT = {"10": 0, "11": 1, "30": 2, "31": 3, "32": 4, "33": 5, "34": 6}


def resolved_fields(signal):
    """[[group, name, first, last, signed, mul, exp, pi], ...] with absolute 1-based bit numbers."""
    out = []
    if signal == "B1C":
        for group, base, fields in B1C_BLOCKS:
            out += [[group, n, base + a - 1, base + b - 1, sg, mul, ex, pi] for n, a, b, sg, mul, ex, pi in fields]
    else:
        for group, fields in B2A_FIELDS.items():
            out += [[group, n, a, b, sg, mul, ex, pi] for n, a, b, sg, mul, ex, pi in fields]
    return out


def _value(bits, first, last, signed, mul, exp, pi):
    w = last - first + 1
    v = int("".join("1" if b else "0" for b in bits[first - 1:last]), 2)  # bin2dec
    if signed and bits[first - 1]:  # twosComp2dec.m:42-44
        v -= 1 << w
    x = float(v)
    if mul != 1:
        x = x * float(mul)
    if exp != 0:
        x = x * 2.0 ** exp
    if pi:
        x = x * PI
    return x


def eph_init():
    """eph_structure_init: [] is NaN; SatType 0 = []; idValid zeros."""
    e = {f: math.nan for f in EPH_FIELDS}
    e.update(flag=0, SatType=0, n_entered=0, idValid=np.zeros(8, dtype=np.int32))
    return e


def _assign(e, bits, fields, model):
    for name, a, b, sg, mul, ex, pi in fields:
        v = _value(bits, a, b, sg and name != model.unsigned_field, mul, ex, pi)
        if name == "SatType":  # 1 / 2 / 3 name a type; 0 leaves the field (B1C ephemeris.m:92-99)
            if 1 <= v <= 3:
                e["SatType"] = int(v)
        elif name == "SOW":  # if isempty(eph.SOW)
            if math.isnan(e["SOW"]):
                e["SOW"] = v
        elif name != "PageID":
            e[name] = v


def enter_b1c(e, bits, model=REFERENCE):
    """ephemeris(navBitsBin, eph) of B1C; False = the PRN field is outside 1..63 and the frame is not entered."""
    prn = _value(bits, 1, 6, False, 1, 0, False)
    if prn < 1 or prn > 63:  # :68-70
        return False
    e["PRN"] = prn  # :67, ahead of the flag gate
    first = not e["flag"]
    page = _value(bits, 615, 620, False, 1, 0, False)
    for group, base, fields in B1C_BLOCKS:
        if (group == "first" and first) or group == "every" or (group == "page1" and page == 1) or (group == "page3" and page == 3):
            _assign(e, bits[base - 1:], fields, model)
    if page == 1:
        e["PageID1"] = 1.0  # :180
    elif page == 3:
        e["PageID3"] = 3.0  # :215
    if first:
        e["TOW"] = e["HOW"] * 3600 + e["SOH"]  # :232-234
    e["flag"] = 1
    e["n_entered"] += 1
    return True


def enter_b2a(e, bits, model=REFERENCE):
    prn = _value(bits, 1, 6, False, 1, 0, False)
    if prn < 1 or prn > 63:  # :61-64
        return False
    t = str(int(_value(bits, 7, 12, False, 1, 0, False)))
    e["PRN"] = prn
    if t in B2A_ID_SLOT:
        e["idValid"][B2A_ID_SLOT[t]] = int(t)
        _assign(e, bits, B2A_FIELDS[t], model)
    else:
        e["idValid"][7] = int(t)  # :302
        _assign(e, bits, B2A_FIELDS["other"], model)
    e["flag"] = 1
    e["n_entered"] += 1
    return True


# ---- the decoding loops ----------------------------------------------------------------------------------------------------------
def nav_decode_channel(signal, prn, sync_prompt, data_prompt=None, model=REFERENCE):
    """{"frames", "eph", "firstSubFrame", "TOW"} of one channel: BCNAV1decoding.m:100-189 / BCNAV2decoding.m:103-159."""
    b1c = signal == "B1C"
    index = ofs.frame_sync_b1c(sync_prompt, prn)[1] if b1c else ofs.frame_sync_b2a(sync_prompt)[1]
    data = sync_prompt if data_prompt is None else data_prompt
    e = eph_init()
    first, tow = math.inf, math.inf
    frames = []
    for i in index:
        f = decode_b1c_frame(data, int(i), model) if b1c else decode_b2a_frame(data, int(i), model)
        need = CRC1_OK | CRC2_OK if b1c else CRC1_OK
        if not f["status"] & SHORT and f["status"] & need == need:
            if (enter_b1c if b1c else enter_b2a)(e, f["bits"], model):
                f["status"] |= ENTERED
                if math.isinf(first):
                    first, tow = float(i), (e["TOW"] if b1c else e["SOW"])
            else:
                f["status"] |= PRN_RANGE
        frames.append(f)
    return {"frames": frames, "eph": e, "firstSubFrame": first, "TOW": tow}


def nav_fields_ref(signal, messages, model=REFERENCE):
    e = eph_init()
    n = sum((enter_b1c if signal == "B1C" else enter_b2a)(e, np.asarray(m, dtype=np.uint8), model) for m in messages)
    return e, n


def same_eph(got, want):
    """None, or what differs: every field bit-equal, NaN in the same places."""
    for k in ("flag", "SatType", "n_entered"):
        if int(got[k]) != int(want[k]):
            return f"{k}: {got[k]} != {want[k]}"
    if not np.array_equal(np.asarray(got["idValid"]), np.asarray(want["idValid"])):
        return f"idValid: {got['idValid']} != {want['idValid']}"
    for f in EPH_FIELDS:
        a, b = float(got[f]), float(want[f])
        if not ((math.isnan(a) and math.isnan(b)) or (a == b and math.copysign(1, a) == math.copysign(1, b))):
            return f"{f}: {a!r} != {b!r}"
    return None


def same_frames(got, want):
    if len(got) != len(want):
        return f"{len(got)} frames, not {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        for k in ("index", "status", "polarity", "bch1_max", "bch2_max"):
            if int(g[k]) != int(w[k]):
                return f"frame {i}: {k} {g[k]} != {w[k]}"
        if not np.array_equal(g["bits"], w["bits"]):
            return f"frame {i}: bits differ at {np.nonzero(np.asarray(g['bits']) != np.asarray(w['bits']))[0][:8]}"
    return None


# ---- the case builder ------------------------------------------------------------------------------------------------------------
def random_fields(rng, layout, **fixed):
    """Raw integers for every field of `layout` ({name: (first, last)}): random over the full width, `fixed` as given."""
    out = {}
    for name, (a, b) in layout.items():
        out[name] = int(rng.integers(0, 1 << (b - a + 1), dtype=np.uint64))
    out.update(fixed)
    return out


def b1c_message(rng, prn, page, soh=None, **fixed):
    """(bits878 with both CRCs in place, the symbols of the frame) for a random message of page `page`."""
    from bds_amd import synth

    page3 = ("GNSS_ID", "WN_0BGTO", "t_0BGTO", "A_0BGTO", "A_1BGTO", "A_2BGTO")
    page1 = tuple(n for g, _, fields in B1C_BLOCKS if g == "page1" for n, *_ in fields)
    skip = page3 if page == 1 else page1 if page == 3 else page1 + page3  # the two pages' fields share bits
    names = {n: r for n, r in synth.BCNAV1_FIELDS.items() if n not in skip}
    f = random_fields(rng, names, PRN=prn, PageID=page, **fixed)
    if soh is not None:
        f["SOH"] = soh
    # IODC's last bit is IODE's first (the reference's ranges): write IODE after IODC, as pack_bcnav1_fields does in dict order
    bits = synth.pack_bcnav1_fields(**f)
    sym = synth.bcnav1_symbols(bits, fill=rng.integers(0, 2, 864))
    bits[590:614] = crc_bits(bits[14:590])
    bits[854:878] = crc_bits(bits[614:854])
    return bits, sym


def b2a_message(rng, prn, mes_type, **fixed):
    """(bits288 with the CRC, the 3000 one-millisecond symbols) for a random message of type `mes_type`."""
    from bds_amd import synth

    layout = dict(synth.BCNAV2_HEAD, **synth.BCNAV2_FIELDS.get(mes_type, {}))
    layout.pop("MesType")
    f = random_fields(rng, layout, PRN=prn, **fixed)
    b = synth.pack_bcnav2_fields(mes_type, **f)
    return np.concatenate([b, crc_bits(b)]), synth.bcnav2_symbols(b)


def noise_like(rng, n):
    """A prompt series without structure: random signs, magnitudes spread over a decade."""
    return rng.choice([-1.0, 1.0], n) * rng.uniform(300.0, 3000.0, n)


def place(series, index, symbols, rng, sign=1.0):
    """Write `symbols` (+-1) into `series` from the 1-based `index` on, with random magnitudes; sign = -1 inverts them."""
    s = np.asarray(symbols, dtype=np.float64)
    series[index - 1:index - 1 + s.size] = sign * s * rng.uniform(300.0, 3000.0, s.size)


def b1c_pilot(rng, n, prn, starts):
    """A pilot prompt series with the PRN's secondary code at each 1-based start."""
    p = noise_like(rng, n)
    for i in starts:
        place(p, i, ocodes.generate_2nd_code(int(prn)), rng)
    return p


def symbol_of_nav_bit(k):
    """0-based position, among the 1800 symbols of a B-CNAV1 frame, of bit k (0-based, 14 <= k < 878) of decodedNav."""
    if k < 614:
        q = k - 14
        rows = [r for r in range(36) if (r + 1) not in FRAME3_ROWS]
    else:
        q = k - 614
        rows = [r - 1 for r in FRAME3_ROWS]
    return 72 + (q % 48) * 36 + rows[q // 48]
