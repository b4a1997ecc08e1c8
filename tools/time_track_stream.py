#!/usr/bin/env python3
"""Time cfg4 as one piece -- 12 channels x 3 600 wide-band epochs at 99.375 MS/s from a raw int8 file (bench.py's
tracking_full leg) -- with the record held as one window and streamed under resident limits:
    python tools/time_track_stream.py [--limits 0,256,1024,4096] [--repeats 5] [--epochs 3600] [--dir DIR]
--limits: MiB per run, 0 = no limit (one window).  Per limit and repeat: the wall time of the tracking() call and the library's own
total_ms (the epoch loop, loads that fall inside it included), then median and max - min of the repeats; pieces, the largest resident
byte count, the bytes loaded and the repeated batches of the last repeat; and the SHA-256 of every result array, so that runs --
also of different libraries -- can be compared bit for bit.  BDS_LIB_PATH selects the library (a build of another commit knows only
--limits 0): run the tool once per library.  The record (3.6 GB, written to --dir before the clock starts) is removed at the end."""
import argparse
import hashlib
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def digest(res):
    h = hashlib.sha256()
    for r in res:
        for f in sorted(vars(r)):
            v = getattr(r, f)
            h.update(f.encode())
            h.update(np.ascontiguousarray(v).tobytes() if isinstance(v, np.ndarray) else repr(v).encode())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--limits", default="0,256,1024,4096")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=3600)
    ap.add_argument("--dir", default=os.environ.get("BDS_BENCH_TMP", tempfile.gettempdir()))
    a = ap.parse_args()
    import bds_amd
    import bench

    base = bds_amd.init_settings_b1c(samplingFreq=99.375e6, IF=14.58e6, acqSatelliteList=list(range(1, 64)), acqCohT=10, pilotACQflag=1)
    s, ch, blocks, order, shift, n, spc = bench.cfg4_record(base, a.epochs)
    fd, path = tempfile.mkstemp(prefix="bds_cfg4_", suffix=".bin", dir=a.dir)
    os.close(fd)
    try:
        bench.write_record(path, blocks, order, shift, n)
        ctx = bds_amd.get_context(0)
        print(f"# library {os.environ.get('BDS_LIB_PATH', 'libbds_mi355x.so (in-tree release build)')}")
        print(f"# {len(ch)} channels x {a.epochs} WB epochs, fs {s.samplingFreq / 1e6:g} MS/s, record {n / 1e9:.3f} GB at {path}")
        bds_amd.tracking(path, ch, s.copy(msToProcess=100), mode="WB")  # warm-up: code tables, kernels, the file in the page cache
        first = None
        for mib in [int(v) for v in a.limits.split(",")]:
            kw = {"resident_limit": mib << 20} if mib else {}
            wall, own = [], []
            for r in range(a.repeats):
                t0 = time.perf_counter()
                res, _ = bds_amd.tracking(path, ch, s, mode="WB", **kw)
                wall.append(time.perf_counter() - t0)
                own.append(ctx.timing()["total_ms"])
                print(f"limit {mib} MiB repeat {r}: wall {wall[-1]:.4f} s, total_ms {own[-1]:.2f}")
            info = ctx.track_stream_info() if hasattr(ctx._lib, "bds_track_stream_info") else {}
            d = digest(res)
            first = first or d
            print(f"limit {mib} MiB: wall s median {np.median(wall):.4f} min {min(wall):.4f} max {max(wall):.4f} max-min {max(wall) - min(wall):.4f};  "
                  f"total_ms median {np.median(own):.2f} max-min {max(own) - min(own):.2f};  completed {sorted({int(q.completed) for q in res})}  "
                  f"loaded {ctx.track_loaded_bytes()} bytes  {info}")
            print(f"limit {mib} MiB: results sha256 {d}  {'= first run' if d == first else 'DIFFERS from the first run'}")
    finally:
        if os.path.exists(path):
            os.remove(path)


if __name__ == "__main__":
    main()
