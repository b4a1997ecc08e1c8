#!/usr/bin/env python3
"""Read the numbers of the reference's navigation decoders -- literals the reference itself ships -- into
tests/golden/nav_tables.json, so that the restatement of tests/nav_cases.py (and through it the library's parser) is pinned
against the reference's own bit ranges and scale factors; a transcription slip in either would otherwise go unseen.

    python tests/golden/make_nav_tables.py <the reference's BDS3_B1C_B2a directory>

The JSON holds names and numbers only:
  bch21_feedback, bch51_feedback      BCH21_6Decoding.m:62, BCH51_8Decoding.m:60
  thresholds                          bch21 (:49), bch51 (:47), b2a_sync (BCNAV2decoding.m:97), b1c_sync (BCNAV1decoding.m:91)
  crc_exponents                       comm.CRCDetector([...]) of both decoders (equal)
  frame3_rows                         Frame3Colum (BCNAV1decoding.m:147)
  fields.B1C / fields.B2A             [group, name, first bit, last bit, signed, factor, exponent of two, times pi] per
                                      assignment of the two ephemeris.m files; bit numbers are 1-based in the whole message
                                      (block slices such as subFra2Bit = navBitsBin(54:256) are resolved).  group: B1C "first" /
                                      "every" / "page1" / "page3"; B2a the message type, "other" for the otherwise branch.
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def read(ref, path):
    with open(os.path.join(ref, path)) as f:
        return f.read()


def vector(text, name):
    m = re.search(r"^\s*" + re.escape(name) + r"\s*=\s*\[([\d\s]+)\]\s*;", text, re.M)
    assert m, name
    return [int(t) for t in m.group(1).split()]


def scalar(text, name):
    m = re.search(r"^\s*" + re.escape(name) + r"\s*=\s*([\d.]+)\s*;", text, re.M)
    assert m, name
    return int(m.group(1))


ASSIGN = re.compile(r"^\s*(?:eph\.)?(\w+)\s*=\s*(bin2dec|twosComp2dec)\(\s*(\w+)\(\s*(\d+)\s*(?::\s*(\d+)\s*)?\)\s*\)(.*?);", re.M)
SLICE = re.compile(r"^\s*(\w+)\s*=\s*(\w+)\(\s*(\d+)\s*:\s*(\d+)\s*\)\s*;")


def fields(text, group_of_line):
    """Walk the file line by line: block slices set the base of their variable, group_of_line names the branch."""
    base = {"navBitsBin": 0}
    group, out = None, []
    for line in text.splitlines():
        code = line.split("%")[0] if not line.lstrip().startswith("%%") else line
        g = group_of_line(line, group)
        if g == "stop":
            break
        group = g
        m = SLICE.match(code)
        if m and m.group(2) in base:
            base[m.group(1)] = base[m.group(2)] + int(m.group(3)) - 1
            continue
        m = ASSIGN.match(code + ("" if code.rstrip().endswith(";") else ";"))
        if not m or group is None:
            continue
        name, fn, var, a, b, tail = m.groups()
        a = int(a)
        b = int(b) if b else a
        exp = re.search(r"\*\s*2\^\(\s*(-?\d+)\s*\)", tail)
        mul = re.search(r"\*\s*(\d+)(?!\s*\^)\b", tail)
        out.append([group, name, base[var] + a, base[var] + b, fn == "twosComp2dec", int(mul.group(1)) if mul else 1,
                    int(exp.group(1)) if exp else 0, bool(re.search(r"\*\s*(bdsPi|gpsPi)", tail))])
    return out


def b1c_group(line, group):
    s = line.strip()
    if s.startswith("if isempty(eph.flag)"):
        return "first" if group is None else "stop"  # the second gate (TOW) ends the fields
    if s.startswith("%% ===== Decode the third subframe"):
        return "every"
    if s.startswith("if PageID == 1"):
        return "page1"
    if s.startswith("elseif PageID == 3"):
        return "page3"
    return group


def b2a_group(line, group):
    s = line.strip()
    m = re.match(r"case\s+(\d+)", s)
    if m:
        return m.group(1)
    if s.startswith("otherwise"):
        return "other"
    if s.startswith("end % switch"):
        return "stop"
    return group


def main(ref):
    d1 = read(ref, "BDS-3_B1C/include/BCNAV1decoding.m")
    d2 = read(ref, "BDS-3_B2a/include/BCNAV2decoding.m")
    b21 = read(ref, "BDS-3_B1C/include/BCH21_6Decoding.m")
    b51 = read(ref, "BDS-3_B1C/include/BCH51_8Decoding.m")
    crc = [re.search(r"comm\.CRCDetector\(\[([\d\s]+)\]\)", t).group(1).split() for t in (d1, d2)]
    assert crc[0] == crc[1]
    lo, step, hi = (int(v) for v in re.search(r"Frame3Colum\s*=\s*(\d+):(\d+):(\d+)\s*;", d1).groups())
    out = {
        "bch21_feedback": vector(b21, "reg1_FeedbackPos"),
        "bch51_feedback": vector(b51, "reg1_FeedbackPos"),
        "thresholds": {
            "bch21": scalar(b21, "threshold"), "bch51": scalar(b51, "threshold"),
            "b2a_sync": int(re.search(r"abs\(tlmXcorrResult\([^)]*\)\)\s*>\s*(\d+)", d2).group(1)),
            "b1c_sync": float(re.search(r"abs\(XcorrResult\)\s*>=\s*([\d.]+)", d1).group(1)),
        },
        "crc_exponents": [int(v) for v in crc[0]],
        "frame3_rows": list(range(lo, hi + 1, step)),
        "fields": {
            "B1C": fields(read(ref, "BDS-3_B1C/include/ephemeris.m"), b1c_group),
            "B2A": fields(read(ref, "BDS-3_B2a/include/ephemeris.m"), b2a_group),
        },
    }
    path = os.path.join(HERE, "nav_tables.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print(path, len(out["fields"]["B1C"]), "B1C and", len(out["fields"]["B2A"]), "B2a assignments")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
