#!/usr/bin/env python3
"""Noise-only deepMetric of the weak-signal acquisition rule, on the NumPy model of tests/deep_cases.py (no GPU): records of
Gaussian noise alone (sigma 20, int8), one PRN, K = 1, 4, 16 and 64 blocks, B2a at 25 MS/s with 11 Doppler bins and B1C at
12.5 MS/s with 9.  The largest value ever seen is what a caller's threshold has to clear.

  python tools/deep_noise_floor.py [--seeds 20] [--out profiles/deep_noise_floor.txt]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KS = (1, 4, 16, 64)


def table(seeds):
    import deep_cases as dc

    lines = ["noise-only deepMetric = (S_peak - mu) / (S_sec - mu) of the NumPy model (tests/deep_cases.py); records of N(0, 20) noise, int8",
             f"{seeds} seeds per row: min / median / max", ""]
    for name, s in (("B2a 25 MS/s, D = 11 (band 2 kHz, step 400 Hz), PRN 21", dc.b2a_settings([21])),
                    ("B1C 12.5 MS/s, D = 9 (band 200 Hz, step 50 Hz), PRN 7", dc.b1c_settings([7]))):
        lines.append(name)
        res = dc.noise_floor(s, KS, range(100, 100 + seeds))
        for k in KS:
            v = np.array(res[k])
            lines.append(f"  K = {k:2d}   {v.min():.3f} / {np.median(v):.3f} / {v.max():.3f}")
        lines.append("")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    text = "\n".join(table(a.seeds))
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
