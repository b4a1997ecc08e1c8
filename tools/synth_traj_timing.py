#!/usr/bin/env python3
"""Generation rate of the synthetic IF generator, constant-Doppler path against trajectory path (not a test; bench.py is untouched).

12 B1C satellites at 99.375 MS/s, format 1 (real int8), 2^30 samples into device memory:
    const         bds_synth_dev of this build
    parent        bds_synth_dev of a build of the parent commit (--parent-lib PATH; without it the arm is "not measured")
    trajectory    bds_synth_traj_dev of this build, on an orbit-driven trajectory of the same 12 satellites (seg_log2 17)
The arms alternate within one process (parent, const, trajectory, parent, ...): --warmup rounds untimed, then --reps rounds; per arm
the median and the spread of the kernel time (the library's own device events, bds_get_timing.forward_ms) and of the wall time of
the call (it returns after a stream synchronise).  The records of `const` and `parent` are compared byte for byte.

    python tools/synth_traj_timing.py [--parent-lib libbds_parent.so] [--log2 30] [--reps 7] [--out profiles/synth_traj_timing.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--log2", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "synth_traj_timing.txt"))
    a = ap.parse_args()

    import torch

    import bds_amd
    from bds_amd import native, synth

    import synth_traj_cases as tc

    n = 1 << a.log2
    s = bds_amd.init_settings_b1c(samplingFreq=99.375e6, IF=24.58e6)
    rng = np.random.default_rng(1)
    spc = 993750
    prns = list(range(19, 31))
    const_sats = [synth.Sat(p, float(rng.uniform(-4000, 4000)), float(rng.uniform(0, spc)), float(rng.uniform(0, 6.28)), 45.0) for p in prns]
    scn = tc.pc.make_scenario("B1C", 12, 8, seed=3, prns=prns)
    traj = synth.trajectory(s, scn.ephs, scn.rx, n, scn.tow, -0.39)
    traj_sats = [synth.Sat(p, 0.0, 0.0, t.phase, 45.0) for p, t in zip(prns, const_sats)]
    print("trajectory:", traj.segs.shape, "segments")
    ctx = bds_amd.get_context(0)

    # the parent build through its own handle: the entries of this measurement only
    parent = None
    if a.parent_lib:
        L = C.CDLL(os.path.abspath(a.parent_lib))
        L.bds_create.restype, L.bds_create.argtypes = C.c_void_p, [C.c_int]
        L.bds_last_error.restype, L.bds_last_error.argtypes = C.c_char_p, [C.c_void_p]
        L.bds_get_timing.restype, L.bds_get_timing.argtypes = C.c_int, [C.c_void_p, C.POINTER(native.Timing)]
        L.bds_synth_dev.restype = C.c_int
        L.bds_synth_dev.argtypes = [C.c_void_p, C.POINTER(native.Settings), C.c_int, C.POINTER(native.SynthSat), C.POINTER(native.SynthOpts),
                                    C.c_int64, C.c_int64, C.c_void_p, C.c_size_t]
        parent = (L, L.bds_create(0))
        if not parent[1]:
            raise SystemExit("the parent build gave no context: " + L.bds_last_error(None).decode())

    bufs = {k: torch.empty(n, dtype=torch.int8, device="cuda:0") for k in ("const", "parent", "trajectory") if k != "parent" or parent}
    cs = native.pack_settings(s)

    def run(arm):
        t0 = time.perf_counter()
        if arm == "parent":
            arr, o, _ = native.pack_synth(const_sats, 1)
            L, h = parent
            if L.bds_synth_dev(h, C.byref(cs), 12, arr, C.byref(o), 0, n, C.c_void_p(bufs[arm].data_ptr()), n) != 0:
                raise SystemExit("parent bds_synth_dev: " + L.bds_last_error(h).decode())
            wall = time.perf_counter() - t0
            t = native.Timing()
            L.bds_get_timing(h, C.byref(t))
            return t.forward_ms, wall * 1e3
        if arm == "const":
            ctx.synth_dev(s, const_sats, 0, n, 1, bufs[arm])
        else:
            ctx.synth_traj_dev(s, traj_sats, traj, 0, n, 1, bufs[arm])
        wall = time.perf_counter() - t0
        return ctx.timing()["forward_ms"], wall * 1e3

    arms = [k for k in ("parent", "const", "trajectory") if k in bufs]
    times = {k: [] for k in arms}
    for r in range(a.warmup + a.reps):
        for arm in arms:
            k_ms, w_ms = run(arm)
            if r >= a.warmup:
                times[arm].append((k_ms, w_ms))
    same = bool(torch.equal(bufs["const"], bufs["parent"])) if parent else None

    lines = ["# tools/synth_traj_timing.py on %s: 12 B1C satellites, 99.375 MS/s, format 1, 2^%d samples into device memory" % (ctx.device_name(), a.log2),
             "# %d warm-up rounds, %d timed rounds, the arms alternating in one process; kernel = the library's device events" % (a.warmup, a.reps),
             "arm          kernel ms median (min .. max)       Gsample/s   call wall ms median"]
    med = {}
    for arm in arms:
        k = np.array([t[0] for t in times[arm]])
        w = np.array([t[1] for t in times[arm]])
        med[arm] = float(np.median(k))
        lines.append("%-12s %9.3f (%9.3f .. %9.3f)   %9.3f   %9.3f" % (arm, np.median(k), k.min(), k.max(), n / np.median(k) / 1e6, np.median(w)))
    if parent:
        lines.append("const / parent kernel time: %.4f (the records are %s)" % (med["const"] / med["parent"], "byte-identical" if same else "DIFFERENT"))
    else:
        lines.append("const / parent: not measured (no --parent-lib)")
    lines.append("trajectory / const kernel time: %.4f (rate ratio %.4f)" % (med["trajectory"] / med["const"], med["const"] / med["trajectory"]))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
