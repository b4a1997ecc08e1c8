#!/usr/bin/env python3
"""Timing of the tone excisor on one MI355X against a device-to-device copy of the same record, taken in the same process at the
same size (profiles/notch_timing.txt keeps a run).  The byte model: the excisor reads the record twice and
writes it once where a copy reads once and writes once -- 1.5 x the copy out of place and in place alike (every line changes),
0.5 x for an estimate-only call.  Per sample and tone each pass adds a 32-bit multiply-add for the phase, one LDS lookup and 2 - 8
integer multiply-adds, so from some tone count on the kernels are bound by those, not by memory; the tool says where.

Cases: int8 real and int8 I/Q (noise alone from make_if_device: the kernels' work does not depend on the samples); 1, 2 and 8
tones; B = 1024; out of place, in place and estimate-only.  Wall clock around calls that end in a device synchronise; one
warm-up, then the median (and best) of --reps.

  python tools/notch_timing.py [--seconds 27] [--reps 5] [--out profiles/notch_timing.txt]"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS = 99.375e6
BLOCK = 1024


def timed(f, reps):
    ts = []
    for i in range(reps + 1):  # (the first is the warm-up)
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    ts = ts[1:]
    return float(np.median(ts)), min(ts)


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        keep = [ln.strip() for ln in out.splitlines() if "GPU[0]" in ln and ("sclk" in ln or "mclk" in ln or "fclk" in ln)]
        return "; ".join(keep) if keep else "not reported"
    except Exception as e:  # noqa: BLE001
        return f"not available ({type(e).__name__})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=27.0, help="record length (the blanker's timing size)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import bds_amd

    ctx = bds_amd.get_context(0)
    n = int(round(a.seconds * FS))
    lines = [f"tone excisor timing on {ctx.device_name()}: {n} samples ({a.seconds:g} s at 99.375 MS/s), B = {BLOCK}",
             f"wall clock around synchronous calls, one warm-up, median / best of {a.reps}; clocks before: {clocks()}",
             "yardstick: torch copy_ (hipMemcpyDtoD) of the same record in the same process; byte model: 1.5 x out of place and in place, 0.5 x estimate-only"]

    def sync():
        torch.cuda.synchronize()

    for name, file_type, iq in (("int8 real", 1, 0), ("int8 I/Q", 2, 1)):
        s = bds_amd.init_settings_b2a(samplingFreq=FS, fileType=file_type)
        per = 2 if iq else 1
        rec = torch.empty(n * per, dtype=torch.int8, device="cuda:0")
        step = 1 << 28
        for first in range(0, n, step):  # (generated in slices: the samples do not depend on the slicing)
            m = min(step, n - first)
            ctx.synth_dev(s, [], first, m, 2 if iq else 1, rec[first * per:(first + m) * per], iq_sign=iq)
        out = torch.empty_like(rec)
        t_copy, t_copy_best = timed(lambda: (out.copy_(rec), sync()), a.reps)
        nbytes = n * per
        lines.append(f"{name}: record of {nbytes} bytes; copy_ {t_copy * 1e3:.3f} / {t_copy_best * 1e3:.3f} ms = {2 * nbytes / t_copy / 1e12:.2f} TB/s read + written")
        saved = rec.clone()
        for k in (1, 2, 8):
            # k tones spread over the band, off every multiple of the block rate
            # (and off the simple fractions of fs: at fs / 4 or at DC the lanes of a wave, 16 or 8 samples apart, all look up the same
            # table entry, which the LDS broadcasts -- a first version of this tool measured that and found no bank conflict at all)
            tones = [(-0.45 + 0.9 * (j + 0.37) / k) * FS + 137.0 for j in range(k)] if iq else [(0.02 + 0.46 * (j + 0.37) / k) * FS + 137.0 for j in range(k)]
            steps = [bds_amd.notch_step(f, FS) for f in tones]
            # (Context.notch with want_est=False: the 2.6e6 x k estimates stay on the device; bringing them to the host, as notch_tones
            # does for its report, costs a copy of 21 MB per tone into pageable memory on top of these times)
            for kind, kw, model in (("out of place", {"out": out}, 1.5), ("in place", {"out": rec}, 1.5), ("estimate only", {"apply": False}, 0.5)):
                def call():
                    ctx.notch(s, rec, steps, 10, want_est=False, **kw)

                t, tb = timed(call, a.reps)
                lines.append(f"  {k} tone{'s' if k > 1 else ' '} {kind:13s}: {t * 1e3:.3f} / {tb * 1e3:.3f} ms = {n / t / 1e9:.1f} Gsample/s; {t / t_copy:.2f} x the copy (byte model {model:.2f})")
                if kind == "in place":
                    rec.copy_(saved)
                    sync()
        del rec, out, saved
        torch.cuda.empty_cache()
    lines.append(f"clocks after: {clocks()}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
