#!/usr/bin/env python3
"""Kernel time of the correlation function (bds_corr_function_dev) on one MI355X on a cfg4-shaped input -- 12 wide-band items at
99.375 MS/s, blksize ~ 993 750, the record generated in device memory -- for T = 3, 9, 33 and 128 taps (128 is the most a call
takes) against the tracking correlator's open-loop kernel (bds_track_correlate, three taps per pass) on the same items.  Both times are the kernels alone, between hipEvents on the library's stream (bds_get_timing search_ms): no upload,
no download.  A warm-up call, then the median of --reps timed calls.

  python tools/corrfn_timing.py [--reps 7] [--out profiles/corrfn_timing.txt]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAPS = (3, 9, 33, 128)
CHUNK = 2048  # samples per workgroup of k_corrfn (csrc/bds_corrfn.hip, kCfChunk)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bds_amd
    from bds_amd.synth import Sat, make_if_device

    fs = 99.375e6
    s = bds_amd.init_settings_b1c(samplingFreq=fs, IF=14.58e6, pilotTRKflag=2, numberOfChannels=12)
    spc = 993750
    rng = np.random.default_rng(4)
    prns = [3, 7, 12, 19, 22, 27, 30, 34, 38, 41, 45, 50]
    sats = [Sat(p, float(rng.uniform(-3000, 3000)), float(rng.uniform(0, spc)), float(rng.uniform(0, 6.28)), 45.0) for p in prns]
    rec = make_if_device(s, sats, 2 * spc + 4096, out="torch")
    st = []
    for sat in sats:
        cf = s.IF + round(sat.doppler / 25) * 25
        code_freq = s.codeFreqBasis - (cf - s.IF) / s.carrFreqBasis * s.codeFreqBasis
        st.append([float(int(np.ceil(sat.delay))), float(int(np.ceil(s.codeLength / (code_freq / fs)))), 0.0, code_freq, 0.0, float(cf)])
    st = np.array(st)
    prn = np.array(prns, dtype=np.int32)
    ctx = bds_amd.get_context(0)
    host = rec.cpu().numpy()
    spc_el = s.dllCorrelatorSpacing

    def median_ms(call):
        call()  # warm-up
        ts = []
        for _ in range(a.reps):
            call()
            ts.append(ctx.timing()["search_ms"])
        return float(np.median(ts)), float(np.min(ts))

    lines = [f"correlation function, kernel time on {ctx.device_name()}: 12 wide-band items at 99.375 MS/s, blksize {int(st[:, 1].min())} .. "
             f"{int(st[:, 1].max())}; hipEvents around the kernels alone, median (best) of {a.reps} calls after a warm-up"]
    med, best = median_ms(lambda: ctx.track_correlate(s, host, prn, st))
    parent = med * 1e3 / (12 * 3)
    lines.append(f"tracking correlator, open loop (k_trk_correlate_open + k_trk_reduce_open, 3 taps per pass): {med:.3f} ({best:.3f}) ms"
                 f" = {parent:.2f} us per item and tap")
    per_tap = {}
    for T in TAPS:
        taps = np.array([-spc_el, 0.0, spc_el]) if T == 3 else np.linspace(-1.6, 1.6, T)
        med, best = median_ms(lambda: ctx.corr_function(s, rec, prn, st, taps))
        per_tap[T] = med * 1e3 / (12 * T)
        lines.append(f"k_corrfn + k_corrfn_reduce, T = {T:3d} taps: {med:.3f} ({best:.3f}) ms = {per_tap[T]:.2f} us per item and tap"
                     f"  ({parent / per_tap[T]:.1f} x cheaper per tap than the tracking correlator)")
    z3 = ctx.corr_function(s, rec, prn, st, [-spc_el, 0.0, spc_el])
    sums = ctx.track_correlate(s, host, prn, st).reshape(12, 3, 3, 2)
    err = np.abs(z3 - (sums[..., 0] + 1j * sums[..., 1])).max() / np.abs(z3[:, 0, 1]).min()
    lines.append(f"the two agree at the tracker taps to {err:.1e} of the smallest |P|")
    # index-step terms per chunk and tap: half-chip steps (data and pilot share them) and BOC(6,1) twelfths
    inc = 2 * s.codeFreqBasis / fs
    lines.append(f"index-step terms per {CHUNK}-sample chunk and tap: {CHUNK * inc:.0f} BOC(1,1) + {CHUNK * inc * 6:.0f} BOC(6,1) = {CHUNK * inc * 7:.0f}"
                 f" (x T taps in phase 2) against {CHUNK} carrier wipe-offs in phase 1")
    assert per_tap[33] < parent, "per tap, T = 33 must be cheaper than the tracking correlator's three taps per pass"
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
