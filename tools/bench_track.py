#!/usr/bin/env python3
"""Tracking timing (BASELINE.json configs[3] shape, shortened): B1C wide-band tracking, 12 channels,
fs = 99.375 MS/s, N 10-ms epochs on a synthetic int8 record resident in HBM.
    python tools/bench_track.py [--epochs 100] [--mode WB|NB|B2A] [--format int8,int8iq,int16,int16iq] [--repeats 1]
Prints ms/epoch, samples/s and GB/s on the record read, one line per record format (real or I/Q, int8 or -- settings.dataType
'int16' -- int16: the same noise values, so the formats differ in the bytes a sample takes only), median / min / max over
--repeats timed calls.  (Noise-only record: the cost per epoch does not depend on lock.)  BDS_LIB_PATH selects the library: a
build of an earlier commit takes the int8 formats."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bds_amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--epochs", type=int, default=100)
ap.add_argument("--mode", default="WB")
ap.add_argument("--channels", type=int, default=12)
ap.add_argument("--format", default="int8")
ap.add_argument("--repeats", type=int, default=1)
a = ap.parse_args()
rng = np.random.default_rng(1)
for fmt in a.format.split(","):
    iq, w16 = fmt.endswith("iq"), fmt.startswith("int16")
    kw = dict(fileType=2 if iq else 1, dataType="int16" if w16 else "schar")
    if a.mode == "B2A":
        s = bds_amd.init_settings_b2a(msToProcess=a.epochs, numberOfChannels=a.channels, **kw)
        spc = 99375
    else:
        s = bds_amd.init_settings_b1c(samplingFreq=99.375e6, IF=14.58e6, msToProcess=a.epochs * 10,
                                      numberOfChannels=a.channels, pilotTRKflag=2 if a.mode == "WB" else 1, **kw)
        spc = 993750
    n = (a.epochs + 2) * spc
    base = min(n, 202 * spc)  # long records repeat a 202-epoch noise block (timing does not depend on the data)
    x = np.clip(np.rint(np.random.default_rng(1).normal(0, 20, base * (2 if iq else 1))), -127, 127).astype(np.int8)
    if base < n:
        x = np.tile(x, n // base + 1)[:n * (2 if iq else 1)]
    if w16:
        x = x.astype(np.int16) * 256
    ch = [SimpleNamespace(PRN=p, acquiredFreq=s.IF + 100.0 * i, codePhase=float(1000 * i + 1), codeFreq=s.codeFreqBasis, status="T")
          for i, p in enumerate(range(1, a.channels + 1))]
    ctx = bds_amd.get_context(0)
    bds_amd.tracking(x, ch, s, mode=a.mode)  # warm-up (includes H2D)
    dev, walls = [], []
    for _ in range(max(a.repeats, 1)):
        t0 = time.perf_counter()
        res, _ = bds_amd.tracking(x, ch, s, mode=a.mode)
        walls.append(time.perf_counter() - t0)
        dev.append(ctx.timing()["total_ms"])
    dev_ms = float(np.median(dev))
    samples = sum(np.diff(r.absoluteSample).sum() + spc for r in res)
    print(json.dumps({"mode": a.mode, "format": fmt, "channels": a.channels, "epochs": a.epochs, "repeats": len(dev), "device_ms": dev_ms,
                      "ms_per_epoch": dev_ms / a.epochs, "ms_per_epoch_min": min(dev) / a.epochs, "ms_per_epoch_max": max(dev) / a.epochs,
                      "wall_s_incl_h2d": float(np.median(walls)), "Msamples_per_s": samples / dev_ms / 1e3,
                      "record_read_GBps": samples * x.itemsize * (2 if iq else 1) / dev_ms / 1e6,
                      "completed": [r.completed for r in res]}))
