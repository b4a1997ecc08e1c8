#!/usr/bin/env python3
"""Time of the position fix on one MI355X, device stage and host chain separately (information only: no target is set; this is
a capability, not a throughput feature).  Two configurations of 12 B1C channels x 3700 code periods (37 s, cfg4's length):

    180 measurement epochs      navSolPeriod = 200 ms, the reference's default
    36 000 measurement epochs   navSolPeriod = 1 ms

Per configuration: the kernel k_pvt_meas alone (hipEvents on the library's stream, bds_get_timing search_ms), the whole
bds_pvt_measure call (upload of the three series, kernel, download; host wall clock incl. ctypes marshalling) and bds_pvt_solve
(host C++, wall clock).  A warm-up call, then the median of --reps calls.

  python tools/pvt_timing.py [--reps 9] [--out profiles/pvt_timing.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bds_amd
    import pvt_cases as pc
    from bds_amd import native

    ctx = bds_amd.get_context(0)
    lines = [f"position fix on {ctx.device_name()}: 12 B1C channels x 3700 code periods at 53 MS/s; median (min) of {a.reps} calls after a warm-up",
             "kernel = k_pvt_meas between hipEvents; measure = bds_pvt_measure, host wall clock incl. upload, download and ctypes; "
             "solve = bds_pvt_solve, host wall clock"]
    for period, want_epochs in ((200, 180), (1, 36000)):
        scn = pc.make_scenario("B1C", 12, 3700, overrides=dict(navSolPeriod=period), seed=7)
        p = native.pvt_plan(scn.settings, scn.status, scn.absoluteSample, scn.ephs, scn.subFrameStart, scn.TOW)
        n_meas = min(want_epochs, p["n_meas"])
        assert n_meas == want_epochs, (n_meas, p["n_meas"])
        args = (scn.settings, p["ready"], scn.absoluteSample, scn.codeFreq, scn.remCodePhase, scn.ephs, scn.subFrameStart, scn.TOW,
                p["sampleStart"], p["measSampleStep"], n_meas)
        tt, sp, ck = ctx.pvt_measure(*args)
        kern, call, solve = [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            tt, sp, ck = ctx.pvt_measure(*args)
            call.append((time.perf_counter() - t0) * 1e3)
            kern.append(ctx.timing()["search_ms"])
            t0 = time.perf_counter()
            sol = native.pvt_solve(scn.settings, scn.prns, p["ready"], p["sampleStart"], p["measSampleStep"], tt, sp, ck)
            solve.append((time.perf_counter() - t0) * 1e3)
        err = np.sqrt((sol["X"] - scn.rx[0]) ** 2 + (sol["Y"] - scn.rx[1]) ** 2 + (sol["Z"] - scn.rx[2]) ** 2)
        fmt = lambda v: f"{np.median(v):.3f} ({np.min(v):.3f}) ms"  # noqa: E731
        lines.append(f"{n_meas:6d} epochs (navSolPeriod {period} ms): kernel {fmt(kern)}, measure {fmt(call)}, solve {fmt(solve)}"
                     f" = {np.median(solve) * 1e3 / n_meas:.2f} us per epoch; every epoch fixed: {bool(np.isfinite(err).all())}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
