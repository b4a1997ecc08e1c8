#!/usr/bin/env python3
"""Worst observed difference of every output of the position fix on one MI355X against the float64 restatement of
tests/pvt_cases.py, on the cases of tests/test_pvt_gpu.py: bds_pvt_measure at its four shapes (also against the restatement in
longdouble, which shows how much of the satPos difference is the restatement's own rounding), bds_post_navigation on the chain
cases, and the fix against the true receiver position of a scenario built without a troposphere.

  python tools/pvt_errors.py [--out profiles/pvt_errors.txt]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bds_amd
    import pvt_cases as pc
    import test_pvt_gpu as tg

    ctx = bds_amd.get_context(0)
    lines = [f"position fix on {ctx.device_name()} against the float64 restatement (tests/pvt_cases.py); worst absolute difference per quantity",
             "tolerances: transmitTime bit-equal, satPos 1e-6 m, satClkCorr 1e-16 s, X Y Z height correctedP 1e-5 m, latitude longitude el az 1e-9 deg,",
             "            DOP 1e-9 relative, dt rawP 1e-5 m + 2 ulp(localTime) c, localTime 2 ulp", "",
             "bds_pvt_measure (signal, n_ch, n, n_meas):"]
    for shape in tg.SHAPES:
        scn, ready, ephs, tow, start, step, want = tg.measure_case(*shape)
        tt, sp, ck = ctx.pvt_measure(scn.settings, ready, scn.absoluteSample, scn.codeFreq, scn.remCodePhase, ephs, scn.subFrameStart, tow,
                                     start, step, shape[3])
        on = np.nonzero(ready == pc.READY)[0]
        ld_dev = ld_ref = 0.0
        for c in on:  # satpos in longdouble at the (bit-equal) transmit times
            pl, _ = pc.satpos(want[0][:, c], ephs[c], shape[0] == "B1C", dtype=np.longdouble)
            ld_dev = max(ld_dev, float(np.abs(sp[:, c] - pl).max()))
            ld_ref = max(ld_ref, float(np.abs(want[1][:, c] - pl).max()))
        lines.append(f"  {shape[0]} {shape[1]:2d} x {shape[2]:4d} x {shape[3]:3d}: transmitTime differs at {int((tt[:, on] != want[0][:, on]).sum())} of "
                     f"{tt[:, on].size}; satPos {np.abs(sp[:, on] - want[1][:, on]).max():.3e} m (device against longdouble {ld_dev:.3e} m, "
                     f"restatement against longdouble {ld_ref:.3e} m); satClkCorr {np.abs(ck[:, on] - want[2][:, on]).max():.3e} s")
    worst = {}
    for name, scn in pc.host_cases().items():
        want = pc.run_reference(scn)[2]
        got, _ = ctx.post_navigation(scn.settings, scn.status, scn.prns, scn.absoluteSample, scn.codeFreq, scn.remCodePhase, scn.ephs,
                                     scn.subFrameStart, scn.TOW)
        for f, v in pc.compare_solutions(got, want).items():
            worst[f] = max(worst.get(f, 0.0), v)
    lines += ["", f"bds_post_navigation on {len(pc.host_cases())} chain cases ({', '.join(pc.host_cases())}):"]
    lines += [f"  {f:15s} {v:.3e}" + (" (relative)" if f == "DOP" else "") for f, v in worst.items()]
    lines += ["", "fix against the true receiver position, useTropCorr = 0 (bound: ||pinv(A)|| sqrt(n_sat) (2 ulp(TOW) c + 1e-4 m)):"]
    for signal, n in (("B1C", 3700), ("B2A", 12200)):
        scn = pc.make_scenario(signal, 5, n, overrides=dict(useTropCorr=0), seed=61)
        want = pc.run_reference(scn)[2]
        got, _ = ctx.post_navigation(scn.settings, scn.status, scn.prns, scn.absoluteSample, scn.codeFreq, scn.remCodePhase, scn.ephs,
                                     scn.subFrameStart, scn.TOW)
        err = np.sqrt((got["X"] - scn.rx[0]) ** 2 + (got["Y"] - scn.rx[1]) ** 2 + (got["Z"] - scn.rx[2]) ** 2)
        bound = min(pc.truth_bound(A, scn.tow, 299792458.0) for A in want["A"])
        lines.append(f"  {signal} 5 x {n}, {err.size} epochs: worst {err.max():.3e} m, bound {bound:.3e} m")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
