#!/usr/bin/env python3
"""Timing of the weak-signal acquisition (bds_acq_deep) on one MI355X, records in HBM (profiles/deep_timing.txt keeps a run):

  B2a at 99.375 MS/s: 63 PRNs x 26 bins x K = 20      B1C at 99.375 MS/s: 4 PRNs x 201 bins x K = 8

Per case: wall time per call (one warm-up, median / best of --reps); kernel time per (PRN, bin, block) cell from a
`rocprofv3 --kernel-trace --stats` run of its own (a child process per case, nothing else traced), split by kernel; beside it the
per-cell time of the library's L-point pair on the same box (acquisition() of the same settings: bds_get_timing's cell_pair_ms /
cells_per_pair) as the yardstick; and, with --probe-lib (tools/build_deep_probe.sh), the column pass's time with its surface stores
compiled out, which gives the share the read-modify-write adds.

  python tools/deep_timing.py [--reps 3] [--prof-dir DIR] [--probe-lib PATH] [--out profiles/deep_timing.txt]"""
import argparse
import glob
import os
import sqlite3
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS = 99.375e6


def case(name):
    import bds_amd

    if name == "b2a":
        s = bds_amd.init_settings_b2a(samplingFreq=FS, acqSatelliteList=list(range(1, 64)), acqSearchBand=5000, acqStep=400)
        return s, 20
    s = bds_amd.init_settings_b1c(samplingFreq=FS, IF=14.58e6, acqSatelliteList=[19, 20, 21, 22], acqSearchBand=5000, acqStep=50, acqCohT=10, pilotACQflag=1)
    return s, 8


def shape(s, k):
    spc = int(np.floor(s.samplingFreq / (s.codeFreqBasis / s.codeLength) + 0.5))
    n = 2 * spc if str(s.signal).upper() == "B2A" else int(np.floor(spc / 10 * (10 + s.acqCohT) + 0.5))
    d = int(np.floor(s.acqSearchBand * 2 / s.acqStep + 0.5)) + 1
    return spc, n, d, len(s.acqSatelliteList)


def record(s, k):
    from bds_amd import synth

    spc, n, _, _ = shape(s, k)
    prn = int(s.acqSatelliteList[0])
    return synth.make_if_device(s, [synth.Sat(prn, 310.0, 0.37 * spc, 1.1, 40.0)], n + (k + 1) * spc, seed=7)


def run_once(name, reps):
    import torch

    import bds_amd

    s, k = case(name)
    x = record(s, k)
    ts = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = bds_amd.acquisition_deep(x, s, k, 1.5)
        ts.append(time.perf_counter() - t)
    return s, k, x, ts[1:], r


def kernel_table(db):
    q = sqlite3.connect(db)
    return [(n, int(c), float(t)) for n, c, t in q.execute("select name,total_calls,total_duration from top_kernels")]


def short(name):
    for key in ("k_cols_deep", "k_rows_inv", "k_cols_fwd<bds::SignalLoader", "k_cols_fwd<bds::CodeLoader", "k_rows_fwd", "k_deep_peak", "k_deep_stats",
                "k_deep_fine", "k_deep_sigpow", "k_make_code"):
        if key in name:
            return key.replace("bds::", "")
    return None


def profile_child(name, prof_dir, lib=None):
    out = os.path.join(prof_dir, name + ("_probe" if lib else ""))
    env = dict(os.environ)
    if lib:
        env["BDS_LIB_PATH"] = lib
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", name, "--", sys.executable, os.path.abspath(__file__), "--child", name]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise RuntimeError(f"profiled child failed ({p.returncode}): {p.stderr[-2000:]}")
    dbs = glob.glob(os.path.join(out, "**", "*_results.db"), recursive=True)
    if not dbs:
        raise RuntimeError("rocprofv3 left no result database under " + out)
    agg = {}
    for n, c, t in kernel_table(dbs[0]):
        key = short(n)
        if key:
            a = agg.setdefault(key, [0, 0.0])
            a[0] += c
            a[1] += t
    for f in dbs:
        os.remove(f)
    return agg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--prof-dir", default=None, help="where the rocprofv3 children write (omit: no kernel times)")
    ap.add_argument("--probe-lib", default=None, help="library of tools/build_deep_probe.sh (omit: no read-modify-write share)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--cases", default="b2a,b1c")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:  # the profiled run: one warm call (plan, code tables), one more
        run_once(a.child, 1)
        return
    import bds_amd

    ctx = bds_amd.get_context(0)
    lines = [f"weak-signal acquisition timing on {ctx.device_name()}, records in HBM; wall clock around calls, one warm-up, median / best of {a.reps}",
             "kernel times: rocprofv3 --kernel-trace --stats of a child process per case (two calls; divided by their cells); one in-flight call at a time", ""]
    for name in a.cases.split(","):
        s, k, x, ts, r = run_once(name, a.reps)
        spc, n, d, p = shape(s, k)
        cells = p * d * k
        lines.append(f"{str(s.signal).upper()} 99.375 MS/s: {p} PRNs x {d} bins x K = {k} = {cells} cells, N = {n}, surfaces {p * d * n * 4 / 2 ** 30:.2f} GiB")
        lines.append(f"  wall per call        : {np.median(ts) * 1e3:.1f} / {min(ts) * 1e3:.1f} ms = {np.median(ts) * 1e6 / cells:.2f} us per cell; detected PRNs {[int(i) + 1 for i in np.nonzero(r.carrFreq)[0]]}")
        ctx.acq_deep_release()
        # yardstick: the library's own pair on the same settings (first N samples of the record)
        bds_amd.acquisition(x, s, verbose=False)
        tm = ctx.timing()
        lines.append(f"  yardstick            : acquisition()'s pair {tm['cell_pair_ms'] * 1e3 / tm['cells_per_pair']:.2f} us per cell "
                     f"(rows_kernel {int(tm['rows_kernel'])}, cols_kernel {int(tm['cols_kernel'])}, half_storage {int(tm['half_storage'])})")
        bds_amd.release_context(0)
        ctx = None
        if a.prof_dir:
            agg = profile_child(name, a.prof_dir)
            tot = sum(v[1] for v in agg.values())
            lines.append(f"  kernels (2 calls)    : {tot / 1e3:.1f} ms = {tot / (2 * cells):.2f} us per cell")
            for key, (c, t) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
                lines.append(f"    {key:28s} {c:7d} launches {t / 1e3:10.2f} ms  {t / (2 * cells):8.3f} us per cell  {100 * t / tot:5.1f} %")
            if a.probe_lib:
                pr = profile_child(name, a.prof_dir, a.probe_lib)
                t1, t0 = agg["k_cols_deep"][1], pr["k_cols_deep"][1]
                model = 8.0 * n
                lines.append(f"  column pass, stores compiled out: {t0 / (2 * cells):.3f} us per cell against {t1 / (2 * cells):.3f}: the surface read-modify-write adds "
                             f"{100 * (t1 - t0) / t1:.1f} % of the pass ({model / 1e6:.2f} MB per cell and block; "
                             f"{model / ((t1 - t0) / (2 * cells) * 1e-6) / 1e12 if t1 > t0 else float('nan'):.2f} TB/s if it were alone)")
        lines.append("")
        ctx = bds_amd.get_context(0)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
