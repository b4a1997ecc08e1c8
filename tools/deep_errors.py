#!/usr/bin/env python3
"""Worst error of the weak-signal acquisition's accumulated surfaces on one MI355X against the NumPy float64 model of
tests/deep_cases.py, on the scenes of tests/test_deep_gpu.py: every value of every row through bds_acq_deep_row, as a fraction of
the tolerance 2e-5 sum_k (max m_k)^2 of its PRN; and deepMetric against the bound that tolerance propagates to.

  python tools/deep_errors.py [--out profiles/deep_errors.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bds_amd
    import deep_cases as dc

    ctx = bds_amd.get_context(0)
    lines = [f"bds_acq_deep on {ctx.device_name()} against the float64 model (tests/deep_cases.py)",
             "surface: worst |S_gpu - S_model| over all D x N values / tolerance (2e-5 sum_k (max m_k)^2); deepMetric: |error| / its bound", ""]
    for name in sorted(dc.GPU_SCENES):
        s, _, k = dc.GPU_SCENES[name]()
        err = dc.surface_errors(name)
        got = dc.run_scene(name, keep_surface=False)
        for prn, r in dc.scene_model(name).items():
            dm = abs(got.deepMetric[prn - 1] - r.deepMetric)
            lines.append(f"{name:18s} K = {k:2d} PRN {prn:2d}  surface {err[prn]:.3e}   deepMetric {r.deepMetric:8.3f} error {dm:.2e} = {dm / dc.deep_metric_bound(r):.3e} of its bound")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
