#!/usr/bin/env python3
"""Read the constants of the reference's position fix -- literals the reference itself ships -- into
tests/golden/pvt_constants.json, so that the restatement of tests/pvt_cases.py (and through it the library) is pinned against the
reference's own numbers; a transcription slip in either would otherwise go unseen.

    python tests/golden/make_pvt_constants.py <the reference's BDS3_B1C_B2a directory>

The JSON holds names and numbers only (every number as the text the reference writes, so that no digit is lost or added):
  bdsPi, OmegaE, mu, F, A_ref_MEO, A_ref_IGSO_GEO   include/satpos.m:32-39 (the B1C and the B2a file must agree)
  half_week                                          include/check_t.m:19
  Omegae_dot                                         Common/e_r_corr.m:21
  ellipsoid5_a, ellipsoid5_finv                      Common/cart2geo.m:22-23, the fifth entries
  topocent_a, topocent_finv                          include/topocent.m:26
  tropo_a_e, tropo_b0, tropo_tlapse                  Common/tropo.m:34-36
  tropo_args                                         the literals of the call in Common/leastSquarePos.m:70-71
  iterations, first_trop                             Common/leastSquarePos.m:33,52
  gate_ms, navSolPeriod, elevationMask, useTropCorr, c, startOffset   per signal: postNavigation.m:49 / :50, initSettings.m
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
NUM = r"(-?[\d.]+(?:[eE][-+]?\d+)?)"


def read(ref, path):
    with open(os.path.join(ref, path)) as f:
        return f.read()


def scalar(text, name):
    m = re.search(r"^\s*" + re.escape(name) + r"\s*=\s*" + NUM + r"\s*;", text, re.M)
    assert m, name
    return m.group(1)


def main(ref):
    out = {}
    sat = [read(ref, d + "/include/satpos.m") for d in ("BDS-3_B1C", "BDS-3_B2a")]
    for name in ("bdsPi", "OmegaE", "mu", "F", "A_ref_MEO", "A_ref_IGSO_GEO"):
        assert scalar(sat[0], name) == scalar(sat[1], name), name
        out[name] = scalar(sat[0], name)
    chk = [scalar(read(ref, d + "/include/check_t.m"), "half_week") for d in ("BDS-3_B1C", "BDS-3_B2a")]
    assert chk[0] == chk[1]
    out["half_week"] = chk[0]
    out["Omegae_dot"] = scalar(read(ref, "Common/e_r_corr.m"), "Omegae_dot")
    geo = read(ref, "Common/cart2geo.m")
    a = re.search(r"^a\s*=\s*\[([\d\s.]+)\]\s*;", geo, re.M).group(1).split()
    f = re.search(r"^f\s*=\s*\[([\d\s./]+)\]\s*;", geo, re.M).group(1).split()
    assert len(a) == 5 and len(f) == 5 and f[4].startswith("1/")
    out["ellipsoid5_a"], out["ellipsoid5_finv"] = a[4], f[4][2:]
    topo = [re.search(r"togeod\(\s*" + NUM + r"\s*,\s*" + NUM + r"\s*,", read(ref, d + "/include/topocent.m")).groups()
            for d in ("BDS-3_B1C", "BDS-3_B2a")]
    assert topo[0] == topo[1]
    out["topocent_a"], out["topocent_finv"] = topo[0]
    trop = read(ref, "Common/tropo.m")
    for name in ("a_e", "b0", "tlapse"):
        out["tropo_" + name] = scalar(trop, name)
    lsq = read(ref, "Common/leastSquarePos.m")
    call = re.search(r"tropo\(sin\(el\(i\) \* dtr\),\s*\.\.\.\s*([^)]*)\)", lsq).group(1)
    out["tropo_args"] = [t.strip() for t in call.split(",")]
    out["iterations"] = scalar(lsq, "nmbOfIterations")
    out["first_trop"] = scalar(lsq, "trop")
    for sig, d in (("B1C", "BDS-3_B1C"), ("B2A", "BDS-3_B2a")):
        post, ini = read(ref, d + "/postNavigation.m"), read(ref, d + "/initSettings.m")
        out[sig] = {"gate_ms": re.search(r"settings\.msToProcess\s*<\s*(\d+)", post).group(1)}
        for name in ("navSolPeriod", "elevationMask", "useTropCorr", "c", "startOffset"):
            out[sig][name] = scalar(ini, "settings." + name)
    path = os.path.join(HERE, "pvt_constants.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(path, len(out), "entries")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
