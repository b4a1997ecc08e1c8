#!/usr/bin/env python3
"""Timing of probe_data on one MI355X against its two floors (the issue's comparison; profiles/probedata_timing.txt keeps a run):
  - the reference window of cfg3: B1C at 99.375 MS/s, int8 real, 10 code periods = 9 937 500 samples (B1C/include/probeData.m:76)
  - the whole cfg4-sized record: 36 s at 99.375 MS/s = 3 577 500 000 int8 samples, generated in device memory by bds_synth_dev
each as (a) the time to read the same bytes once at the achievable HBM rate (6.3 TB/s), (b) the fp32 flop count of the
transforms, nominal 5 N log2 N per segment and as executed, and for the reference window (c) scipy.signal.welch +
numpy.histogram on the host's cores.

  python tools/probe_timing.py [--seconds 36] [--reps 5] [--out profiles/probedata_timing.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.3e12          # B/s achievable (float4 copy)
NFFT, HOP = 32768, 30720
NOMINAL = 5 * NFFT * 15                                   # 5 N log2 N
# as executed per segment (k_probe_segment, real record): 8-point stage 32768 x 8 x (1 window product + 2 products + 2 additions),
# 12 stages x 16384 butterflies x 10 flops, 8 x 2049 x 3 for |X|^2 -- both halves of the spectrum are computed, one is stored
EXECUTED_REAL = 32768 * 8 * 5 + 12 * 16384 * 10 + 8 * 2049 * 3


def timed(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return min(ts), float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=36.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import scipy.signal
    import torch

    import bds_amd
    from bds_amd.synth import make_if_device

    s = bds_amd.init_settings_b1c(samplingFreq=99.375e6, fileType=1, dataType="schar")
    ctx = bds_amd.get_context(0)
    lines = [f"probe_data timing on {ctx.device_name()}; times are wall clock around the call (it returns after its last device work), best / median of {a.reps}"]

    def report(name, n, best, med):
        k = (n - 2048) // HOP
        lines.append(f"{name}: {n} int8 samples, {k} segments: {best * 1e3:.3f} / {med * 1e3:.3f} ms = {n / best / 1e9:.2f} GB/s of record")
        lines.append(f"    floor (a) one read of {n} bytes at {HBM / 1e12:.1f} TB/s: {n / HBM * 1e3:.4f} ms  ({best / (n / HBM):.0f} x)")
        lines.append(f"    floor (b) transforms: nominal 5 N log2 N = {k * NOMINAL / 1e9:.2f} GFLOP, as executed {k * EXECUTED_REAL / 1e9:.2f} GFLOP"
                     f" -> {k * EXECUTED_REAL / best / 1e12:.2f} TFLOP/s fp32 achieved")

    n_ref = 10 * 993750
    rec = make_if_device(s, [], n_ref, out="torch")
    best, med = timed(lambda: bds_amd.probe_data(rec, s), a.reps)
    report("cfg3 reference window (device tensor)", n_ref, best, med)
    x = rec.cpu().numpy()
    best_h, med_h = timed(lambda: bds_amd.probe_data(x, s), a.reps)
    lines.append(f"    the same bytes from host memory (one upload): {best_h * 1e3:.3f} / {med_h * 1e3:.3f} ms")
    xf = x.astype(np.float64)
    w = scipy.signal.windows.hamming(NFFT, sym=True)

    def cpu():
        scipy.signal.welch(xf, 99.375e6, window=w, noverlap=2048, nfft=NFFT, detrend=False, scaling="density")
        np.histogram(x, bins=np.concatenate([[-np.inf], np.arange(-127.5, 128.0), [np.inf]]))

    best_c, med_c = timed(cpu, 3)
    lines.append(f"    (c) scipy.signal.welch + numpy.histogram on this host ({os.environ.get('OMP_NUM_THREADS', '?')} threads allowed): {best_c * 1e3:.1f} / {med_c * 1e3:.1f} ms  ({best_c / best:.1f} x the device)")
    del rec

    n_all = int(round(a.seconds * 99.375e6))
    rec = torch.empty(n_all, dtype=torch.int8, device="cuda:0")
    step = 1 << 28
    t = time.perf_counter()
    for first in range(0, n_all, step):  # (generated in slices: the samples do not depend on the slicing)
        m = min(step, n_all - first)
        ctx.synth_dev(s, [], first, m, 1, rec[first:first + m])
    lines.append(f"cfg4-sized record generated in device memory in {time.perf_counter() - t:.2f} s")
    best, med = timed(lambda: bds_amd.probe_data(rec, s), max(2, a.reps // 2))
    report(f"cfg4-sized record ({a.seconds:g} s, device tensor)", n_all, best, med)
    r = bds_amd.probe_data(rec, s)
    assert int(r.hist_i.sum()) == n_all
    lines.append(f"    histogram total {int(r.hist_i.sum())}, rms {r.rms:.3f}, min {r.min}, max {r.max}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
