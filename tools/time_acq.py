#!/usr/bin/env python3
"""Time bds_acq_run for any settings, with nothing but native.Context and its timing():
    python tools/time_acq.py [--b2a [--b2a-npoint 1]] [--b1c-npoint 1] [--int16] [--set name=value ...] [--prns 19,20 | --prns all] [--repeats 5] [--calls 10] [--sieve-error]
The settings start from init_settings_b1c() (53 MS/s, the reference's B1C/initSettings.m), with --b2a from init_settings_b2a() (99.375 MS/s,
26 bins: `--b2a --prns all` is the grid of BASELINE.json configs[1]); --set overrides fields (numbers are parsed).  --b2a-npoint 1 / 0 sets
the context's switch for the opt-in N-point search of csrc/bds_acq_pfa6.h (bds_acq_set_b2a_npoint; not given: the library's default, and no
call of the entry, so that a library of an earlier commit can be timed); --b1c-npoint 1 / 0 likewise for the opt-in B1C pair of
csrc/bds_acq_pfa31.h (bds_acq_set_b1c_npoint: `--set samplingFreq=30.69e6 --set IF=7.5e6`).  --int16: the block as int16 samples, 256 x the int8 values, under
settings.dataType 'int16' (bds_acq_load16: the float64 view, the L-point pair and the host refinement path); the time of acq_load is printed too.
A synthetic 40 ms block (--b2a: 17 ms) is loaded once and stays in HBM, the code spectra are prepared and one warm-up call runs before the clock
starts.  Per repeat: the mean over --calls calls of the wall time of acq_run and of the library's own total_ms; then the median and
max - min of the repeats.  BDS_LIB_PATH selects the library (a build of another commit, for instance): run the tool once per library.
--sieve-error: also the search grid against the same grid with fp32 storage (BDS_ACQ_FP16=0, test-hooks build), as
tools/sieve_error_cfg3.py reports it at cfg3: worst row-maximum difference relative to the PRN's maximum."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", action="append", default=[], metavar="NAME=VALUE")
    ap.add_argument("--prns", default="19,20")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--seed", type=int, default=53)
    ap.add_argument("--sieve-error", action="store_true")
    ap.add_argument("--b2a", action="store_true")
    ap.add_argument("--b2a-npoint", type=int, choices=(0, 1), default=None)
    ap.add_argument("--b1c-npoint", type=int, choices=(0, 1), default=None)
    ap.add_argument("--int16", action="store_true")
    a = ap.parse_args()
    if a.sieve_error:
        os.environ.setdefault("BDS_LIB_PATH", os.path.join(ROOT, "bds-3-b1c-b2a-sdr-receiver_amd", "libbds_mi355x_hooks.so"))
    import bds_amd
    from bds_amd import synth

    over = {}
    for kv in a.set:
        k, v = kv.split("=", 1)
        try:
            over[k] = int(v)
        except ValueError:
            try:
                over[k] = float(v)
            except ValueError:
                over[k] = v
    prns = list(range(1, 64)) if a.prns == "all" else [int(p) for p in a.prns.split(",")]
    s = (bds_amd.init_settings_b2a if a.b2a else bds_amd.init_settings_b1c)(**over).copy(acqSatelliteList=prns)
    spc = int(round(s.samplingFreq * (1e-3 if a.b2a else 10e-3)))
    sats = [synth.Sat(prns[0], -1730.0, 0.613 * spc, 0.7, 45.0)] + ([synth.Sat(prns[-1], 2210.0, 0.2 * spc, 2.0, 46.0)] if len(prns) > 2 else [])
    x = synth.make_if(s, sats, (17 if a.b2a else 4) * spc, seed=a.seed)
    if a.int16:
        s, x = s.copy(dataType="int16"), x.astype(np.int16) * 256

    def context(env):
        os.environ.update(env)
        c = bds_amd.native.Context(0)
        for k in env:
            del os.environ[k]
        if a.b2a_npoint is not None:
            c.acq_set_b2a_npoint(a.b2a_npoint)
        if a.b1c_npoint is not None:
            c.acq_set_b1c_npoint(a.b1c_npoint)
        c.acq_load(s, x)
        c.acq_prepare(s)
        return c

    c = context({})
    loads = []
    for _ in range(max(a.repeats, 1)):
        t0 = time.perf_counter()
        c.acq_load(s, x)
        loads.append((time.perf_counter() - t0) * 1e3)
    print(f"# acq_load of {x.size} {x.dtype} samples ({x.nbytes / 1e6:.2f} MB): wall ms median {np.median(loads):.3f}  min {min(loads):.3f}  max {max(loads):.3f}")
    res = c.acq_run(s, prn_list=prns)
    tm = c.timing()
    print(f"# library {os.environ.get('BDS_LIB_PATH', 'libbds_mi355x.so (in-tree release build)')}")
    print(f"# fs {s.samplingFreq / 1e6:g} MS/s, {len(prns)} PRNs x {int(tm['n_bins'])} bins, fft_len {int(tm['fft_len'])}, plan {int(tm['plan_l1'])} x {int(tm['plan_l2'])}, "
          f"rows_kernel {int(tm['rows_kernel'])}, cols_kernel {int(tm['cols_kernel'])}, refine_path {int(tm.get('refine_path', -1))}, detected {[p for p in prns if res[0][p - 1] != 0]}")
    wall, own = [], []
    for r in range(a.repeats):
        t0 = time.perf_counter()
        acc = 0.0
        for _ in range(a.calls):
            c.acq_run(s, prn_list=prns)
            acc += c.timing()["total_ms"]
        wall.append((time.perf_counter() - t0) * 1e3 / a.calls)
        own.append(acc / a.calls)
        tm = c.timing()
        print(f"repeat {r}: wall {wall[-1]:.3f} ms per call, total_ms {own[-1]:.3f} (last call: forward {tm['forward_ms']:.3f} search {tm['search_ms']:.3f} refine {tm['refine_ms']:.3f})")
    print(f"wall ms per call: median {np.median(wall):.3f}  min {min(wall):.3f}  max {max(wall):.3f}  max-min {max(wall) - min(wall):.3f}")
    print(f"total_ms per call: median {np.median(own):.3f}  min {min(own):.3f}  max {max(own):.3f}  max-min {max(own) - min(own):.3f}")
    if a.sieve_error:
        nb = int(tm["n_bins"])
        h = c.acq_grid(len(prns), nb)[0].astype(np.float64)
        c.close()
        c = context({"BDS_ACQ_FP16": "0"})
        c.acq_run(s, prn_list=prns)
        assert int(c.timing()["half_storage"]) == 0
        f = c.acq_grid(len(prns), nb)[0].astype(np.float64)
        glob = np.abs(h - f) / f.max(axis=1, keepdims=True)
        print(f"sieve error, {len(prns)} x {nb} rows against fp32 storage: |diff| / PRN maximum  max {glob.max():.3e}  mean {glob.mean():.3e}  (bound 1e-3)")
    c.close()


if __name__ == "__main__":
    main()
