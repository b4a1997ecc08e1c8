#!/usr/bin/env python3
"""Timing of the pulse blanker on one MI355X against a device-to-device copy of the same record, taken in the same process at
the same size (profiles/blank_timing.txt keeps a run).  The byte model: the blanker reads the record twice
and writes it once where a copy reads once and writes once -- 1.5 x the copy out of place; in place it writes only the 16-byte
lines that change and skips the second read of tiles nothing reaches -- about 1.0 x on a sparsely blanked record.

Cases: int8 real and int8 I/Q; out of place and in place; a clean record (noise alone from make_if_device: nothing blanked) and a
jammed one (the scenario's pulse statistics at 99.375 MS/s: 20 000 pairs/s, peak 400, added to the record on the device with torch;
threshold 100, pre = post = 99 samples -- about a quarter of the samples blanked).  Wall clock around calls that end in a device
synchronise; one warm-up, then the median (and best) of --reps.  Then the file path against write_if on the same box, as context.

  python tools/blank_timing.py [--seconds 27] [--reps 5] [--file-seconds 36] [--out profiles/blank_timing.txt]"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS = 99.375e6
BLOCK = 1 << 24  # samples of the interference block that is laid over the record again and again


def timed(f, reps, before=None):
    ts = []
    for i in range(reps + 1):  # (the first is the warm-up)
        if before:
            before()
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
    ap.add_argument("--seconds", type=float, default=27.0, help="record length (36 s is cfg4's 3.6e9 samples)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--file-seconds", type=float, default=36.0, help="length of the file-path comparison (0: skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import bds_amd
    from bds_amd import synth

    ctx = bds_amd.get_context(0)
    n = int(round(a.seconds * FS))
    us = int(round(1e-6 * FS))
    lines = [f"pulse blanker timing on {ctx.device_name()}: {n} samples ({a.seconds:g} s at 99.375 MS/s; cfg4 is 3 577 500 000), threshold 100, pre = post = {us}",
             f"wall clock around synchronous calls, one warm-up, median / best of {a.reps}; clocks before: {clocks()}",
             "yardstick: torch copy_ (hipMemcpyDtoD) of the same record in the same process; model: out of place 1.5 x, in place on a sparse record 1.0 x, 15 % allowed over it"]

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
        p = synth.dme_pulses(s, BLOCK, pairs_per_s=20000, peak=400, f_offset=1e6, seed=7, iq_sign=iq)
        pq = np.rint(np.stack([p.real, p.imag], axis=1).reshape(-1) if iq else p).astype(np.int16)
        for kind in ("clean", "jammed"):
            if kind == "jammed":
                pt = torch.from_numpy(pq).to("cuda:0")
                for first in range(0, nbytes, pq.size):  # the pulses, added on the device and quantised again
                    m = min(pq.size, nbytes - first)
                    seg = rec[first:first + m]
                    seg.copy_((seg.to(torch.int16) + pt[:m]).clamp_(-127, 127).to(torch.int8))
                del pt
                sync()
            saved = rec.clone() if kind == "jammed" else None
            rep = {}

            def oop():
                rep["r"] = bds_amd.blank_pulses(rec, s, threshold=100, pre=us, post=us, out=out)[1]

            def inp():
                rep["r"] = bds_amd.blank_pulses(rec, s, threshold=100, pre=us, post=us, out="inplace")[1]

            t, tb = timed(oop, a.reps)
            r = rep["r"]
            frac = r.fraction
            lines.append(f"  {kind:6s} out of place: {t * 1e3:.3f} / {tb * 1e3:.3f} ms = {n / t / 1e9:.1f} Gsample/s, {3 * nbytes / t / 1e12:.2f} TB/s effective (2 reads + 1 write);"
                         f" {t / t_copy:.2f} x the copy (model 1.50, bound {1.5 * 1.15:.3f}){' ABOVE THE BOUND' if t / t_copy > 1.5 * 1.15 else ''};"
                         f" blanked {100 * frac:.2f} %, {r.n_runs} runs")
            t, tb = timed(inp, a.reps, before=(lambda: (rec.copy_(saved), sync())) if saved is not None else None)
            r = rep["r"]
            moved = nbytes * (1 + (1 if kind == "jammed" else 0) + r.fraction)  # summary read; second read and the changed lines where blanked
            model = "1.00" if kind == "clean" else "between 1.0 and 1.5"
            over = kind == "clean" and t / t_copy > 1.15
            lines.append(f"  {kind:6s} in place:     {t * 1e3:.3f} / {tb * 1e3:.3f} ms = {n / t / 1e9:.1f} Gsample/s, {moved / t / 1e12:.2f} TB/s effective;"
                         f" {t / t_copy:.2f} x the copy (model {model}){' ABOVE THE BOUND' if over else ''}; blanked {100 * r.fraction:.2f} %")
            del saved
        del rec, out
        torch.cuda.empty_cache()
    lines.append(f"clocks after: {clocks()}")

    if a.file_seconds > 0:
        s = bds_amd.init_settings_b2a(samplingFreq=FS, fileType=1)
        m = int(round(a.file_seconds * FS))
        with tempfile.TemporaryDirectory() as d:
            src, dst = os.path.join(d, "rec.bin"), os.path.join(d, "blanked.bin")
            t = time.perf_counter()
            synth.write_if(src, s, [], m)
            t_write = time.perf_counter() - t
            t = time.perf_counter()
            _, r = bds_amd.blank_pulses(src, s, threshold=100, pre=us, post=us, out=dst)
            t_blank = time.perf_counter() - t
            lines.append(f"file path (context, not a bound): {m} int8 samples: write_if {t_write:.2f} s, blank_pulses file -> file {t_blank:.2f} s ({t_blank / t_write:.2f} x),"
                         f" blanked {r.n_blanked}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
