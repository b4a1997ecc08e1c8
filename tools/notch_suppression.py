#!/usr/bin/env python3
"""What the tone excisor leaves behind, computed on the NumPy model of the rule (tests/notch_cases.py; no GPU: the device gives the
same bytes).  A clean record of rounded Gaussian noise, one CW line added and the sum quantised again; the line is notched at
a frequency that is off by 0 / 100 / 1 000 / 3 000 Hz, and again at the frequency notch_refine gives from an estimate-only
pass; the figure is the rms of (notched - clean) in LSB, beside the noise it sits under.  Then two tones 4.5, 8.5 and 16.5 notch widths
apart, notched once and twice (the tones are projected independently and leak about 1 / (pi D) into each other's estimate).

  python tools/notch_suppression.py [--out profiles/notch_suppression.txt]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FS = 25e6
F0 = 6.9e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import conftest  # noqa: F401  (puts the package on the path under its import name)
    import bds_amd
    import notch_cases as nc

    n = 1 << 18
    t = np.arange(n)
    lines = [f"tone excisor: residual of the NumPy model against the clean record, {n} samples at {FS / 1e6:g} MS/s, one line at {F0 / 1e6:g} MHz",
             "rms of (notched - clean) in LSB; 'before': notched at the line's frequency plus the error; 'after': at notch_refine's frequency from an estimate-only pass"]
    for fmt, sigma, amp in (("s8", 6.0, 100.0), ("s16", 300.0, 30000.0)):
        dt = nc.FORMATS[fmt][2]
        s = nc.settings_of(fmt, samplingFreq=FS, IF=6.5e6)
        clean = nc.noise(fmt, n, seed=1, sigma=sigma)
        jam = np.clip(np.rint(clean + amp * np.cos(2 * np.pi * F0 * t / FS + 0.7)), np.iinfo(dt).min + 1, np.iinfo(dt).max).astype(dt)
        lines.append(f"{'int8' if fmt == 's8' else 'int16'} real, sigma = {sigma:g}, CW amplitude {amp:g} (J/N = {10 * np.log10(amp * amp / 2 / sigma ** 2):+.1f} dB); jammed rms error {np.sqrt(np.mean((jam.astype(float) - clean) ** 2)):.1f}")
        for beta in (8, 10, 12):
            B = 1 << beta
            row = []
            for err in (0.0, 100.0, 1000.0, 3000.0):
                steps = [bds_amd.notch_step(F0 + err, FS)]
                out, _ = nc.model(jam, fmt, steps, beta)
                before = np.sqrt(np.mean((out.astype(float) - clean) ** 2))
                _, r = nc.model(jam, fmt, steps, beta, apply=False)
                rep = bds_amd.NotchReport(n_samples=n, n_blocks=r["n_blocks"], n_saturated=0, sum_sq_in=0, sum_sq_out=0,
                                          est=(r["est"][..., 0] + 1j * r["est"][..., 1]) / 256.0, steps=steps, tones=[F0 + err], block=B)
                fine = bds_amd.notch_refine(rep, s)
                out2, _ = nc.model(jam, fmt, [bds_amd.notch_step(fine[0], FS)], beta)
                after = np.sqrt(np.mean((out2.astype(float) - clean) ** 2))
                row.append(f"{err:5.0f} Hz: {before:9.2f} -> {after:7.2f} (refined to within {fine[0] - F0:+6.2f} Hz)")
            lines.append(f"  B = {B:5d} (notch {FS / B / 1e3:6.2f} kHz)  " + "   ".join(row))
    lines.append("two tones of amplitude 50 in int8 noise of sigma 6, D notch widths apart at B = 1024: rms of (notched - clean) after one pass and after a second pass on the output")
    clean = nc.noise("s8", n, seed=2, sigma=6.0)
    for d in (4, 8, 16):
        f1 = F0 + (d + 0.5) * FS / 1024  # (at whole widths the two are orthogonal over a block: the leak is largest half way)
        jam = np.clip(np.rint(clean + 50 * np.cos(2 * np.pi * F0 * t / FS + 0.7) + 50 * np.cos(2 * np.pi * f1 * t / FS + 2.1)), -127, 127).astype(np.int8)
        steps = [bds_amd.notch_step(F0, FS), bds_amd.notch_step(f1, FS)]
        once, _ = nc.model(jam, "s8", steps, 10)
        twice, _ = nc.model(once, "s8", steps, 10)
        lines.append(f"  D = {d + 0.5:4.1f}: {np.sqrt(np.mean((once.astype(float) - clean) ** 2)):6.2f} -> {np.sqrt(np.mean((twice.astype(float) - clean) ** 2)):6.2f}   (1 / (pi D) of 50 = {50 / np.pi / (d + 0.5):.2f})")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
