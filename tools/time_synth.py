#!/usr/bin/env python3
"""What the device generator of synthetic IF records costs (bds_synth / bds_synth_file) -> profiles/r13_synth.txt.

The case: 12 B1C satellites at 99.375 MS/s (cfg4's shape).  Per format (1 real int8, 2 I/Q int8, 3 packed 2+2-bit I/Q), over
`--samples` samples written to /dev/null in the default pieces: the generation kernels' time and the same pieces' device-to-host
copy time (device events of the same call, bds_get_timing: forward_ms / search_ms) and the call's stream time, best and worst of
`--repeats` after one warm-up call.  The kernel is acceptable when a piece is generated in no more than the time its own copy
takes -- the two overlap in bds_synth_file, so then the generator is never what write_if waits for; the verdict is printed per
format.  Then the wall time of write_if for `--long-samples` samples (3.607e9 = BASELINE configs[3]) to a file in --tmp (removed
afterwards) and to /dev/null, synth.make_if on this host for 2^22 samples of the same case, and the measured maxima of the
parity checks of tests/test_synth_gpu.py (clean sum and noise stream against the NumPy restatement).

    python tools/time_synth.py [--out profiles/r13_synth.txt] [--samples N] [--long-samples N] [--repeats R] [--skip-host]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bds_amd  # noqa: E402
from bds_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_synth.txt"))
    ap.add_argument("--samples", type=int, default=1 << 30)
    ap.add_argument("--long-samples", type=int, default=3_607_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tmp", default=tempfile.gettempdir())
    ap.add_argument("--skip-host", action="store_true", help="leave out synth.make_if on the host (15 s here)")
    a = ap.parse_args()

    s = bds_amd.init_settings_b1c(samplingFreq=99.375e6)
    sats = synth.random_sats(np.random.default_rng(4), [1, 4, 9, 14, 19, 20, 27, 35, 46, 58, 60, 63], 993750)
    ctx = bds_amd.get_context(0)
    lines = ["# tools/time_synth.py on %s" % ctx.device_name(),
             "# case: %d B1C satellites at %.3f MS/s, sigma 20; pieces of 64 MiB (packed: 32 MiB), written to /dev/null" % (len(sats), s.samplingFreq / 1e6),
             "# per call of %d samples: kernel = sum of the generation kernels (device events), d2h = sum of the pieces' copies to pinned memory," % a.samples,
             "# stream = first kernel's start to last copy's end; min .. max of %d calls after one warm-up call" % a.repeats,
             "format  bytes/sample  kernel ms          d2h ms             stream ms          kernel ns/sample  Gsample/s  d2h GB/s  kernel <= d2h"]
    kinds = {1: dict(), 2: dict(iq_sign=-1), 3: dict(iq_sign=-1, packed=True)}
    for fmt, kw in kinds.items():
        n = a.samples - a.samples % 2
        synth.write_if("/dev/null", s, sats, min(n, 1 << 26), **kw)  # warm-up: code object, pinned buffers' first touch
        rows = []
        for _ in range(a.repeats):
            synth.write_if("/dev/null", s, sats, n, **kw)
            t = ctx.timing()
            rows.append((t["forward_ms"], t["search_ms"], t["total_ms"]))
        k, c, tot = (np.array(v) for v in zip(*rows))
        bps = {1: 1.0, 2: 2.0, 3: 0.5}[fmt]
        lines.append("%-7d %-13.1f %8.2f .. %-8.2f %8.2f .. %-8.2f %8.2f .. %-8.2f %-17.4f %-10.3f %-9.2f %s" % (
            fmt, bps, k.min(), k.max(), c.min(), c.max(), tot.min(), tot.max(), k.min() * 1e6 / n, n / k.min() / 1e6, n * bps / c.min() / 1e6,
            "yes" if k.min() <= c.min() else "NO (%.1f x the copy)" % (k.min() / c.min())))
    # one long record, as a user would make it
    path = os.path.join(a.tmp, "bds_time_synth_%d.bin" % os.getpid())
    n = a.long_samples
    try:
        t0 = time.perf_counter()
        synth.write_if(path, s, sats, n)
        wall = time.perf_counter() - t0
        t = ctx.timing()
        size = os.path.getsize(path)
    finally:
        if os.path.exists(path):
            os.remove(path)
    assert size == n
    lines.append("write_if, %d samples (format 1, %.2f GB) to a file in %s: %.2f s wall (kernels %.0f ms, copies %.0f ms, stream %.0f ms)"
                 % (n, n / 1e9, a.tmp, wall, t["forward_ms"], t["search_ms"], t["total_ms"]))
    t0 = time.perf_counter()
    synth.write_if("/dev/null", s, sats, n)
    wall = time.perf_counter() - t0
    lines.append("write_if, the same record to /dev/null: %.2f s wall (stream %.0f ms)" % (wall, ctx.timing()["total_ms"]))
    if not a.skip_host:
        t0 = time.perf_counter()
        synth.make_if(s, sats, 1 << 22)
        host = time.perf_counter() - t0
        lines.append("synth.make_if (NumPy) on this host, %d samples of the same case: %.1f s = %.3f Msample/s" % (1 << 22, host, (1 << 22) / host / 1e6))
    # the parity figures of tests/test_synth_gpu.py
    import synth_cases as sc

    nn = 1 << 20
    got = synth.make_if_device(s, sats, nn, first_sample=12345, clean=True)
    ref = sc.clean_record(s, sats, 12345, nn)
    lines.append("clean sum, %d samples from 12 345: max |device - NumPy restatement| = %.3e (bound 8 eps sum(amp) 1.3 = %.3e)"
                 % (nn, np.abs(got - ref).max(), 8 * np.finfo(float).eps * sc.amp_sum(s, sats) * 1.3))
    g_i, g_q = ctx.synth_noise(3550, 2 ** 33 - 5, 1 << 16)
    r_i, r_q = sc.noise_normals(3550, np.arange(2 ** 33 - 5, 2 ** 33 - 5 + (1 << 16), dtype=np.int64))
    lines.append("noise stream, 2^16 draws from 2^33 - 5: max |device - NumPy restatement| = %.3e (bound 1e-13)" % max(np.abs(g_i - r_i).max(), np.abs(g_q - r_q).max()))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
