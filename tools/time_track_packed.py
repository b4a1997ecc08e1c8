#!/usr/bin/env python3
"""Time wide-band tracking of one I/Q record in its two on-disk forms: int8 pairs (settings.fileType 2) and packed 2+2-bit bytes
(fileType 3, a quarter of the size) -- cfg4's shape: 12 channels, B1C wide-band, 99.375 MS/s, 10-ms epochs.
    python tools/time_track_packed.py [--epochs 1200] [--repeats 5] [--limits 0,256] [--dir DIR]
    python tools/time_track_packed.py --profile 2|3 [--epochs 200]      one call from memory, for rocprofv3 --kernel-trace --stats
The record is noise quantised to {+-1, +-3} (sign, and one magnitude threshold at the rms; the cost per epoch does not depend on
lock, tools/bench_track.py): a 50-epoch block repeated.  Both files hold the same samples, the channels start on even and odd
samples.  Per format and limit (MiB of the record resident in HBM, 0 = none: one window) and repeat: the wall time of the
tracking() call from the file and the library's own total_ms (the epoch loop); then median and max - min, the bytes loaded, the
pieces, and the SHA-256 of every result array -- the two formats must agree bit for bit.  The last lines compare the formats.
The files (2.4 GB + 0.6 GB at the default length) are written to --dir before the clock starts and removed at the end."""
import argparse
import hashlib
import os
import sys
import tempfile
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

SPC = 993750  # samples of a 10-ms code period at 99.375 MS/s
BLOCK_EPOCHS = 50
LUT_I = np.array([1, -1, 1, -1, 3, -3, 3, -3, 1, -1, 1, -1, 3, -3, 3, -3], dtype=np.int8)  # B2a/include/unpack_cplx.m:20-21
LUT_Q = np.array([1, 1, -1, -1, 1, 1, -1, -1, 3, 3, -3, -3, 3, 3, -3, -3], dtype=np.int8)


def digest(res):
    h = hashlib.sha256()
    for r in res:
        for f in sorted(vars(r)):
            v = getattr(r, f)
            h.update(f.encode())
            h.update(np.ascontiguousarray(v).tobytes() if isinstance(v, np.ndarray) else repr(v).encode())
    return h.hexdigest()


def noise_block(n_samples, seed=1):
    """(packed uint8 [n / 2], int8 pairs [2 n]) of n complex noise samples: a 2-bit converter with its threshold at the rms."""
    rng = np.random.default_rng(seed)
    g = rng.normal(0.0, 1.0, 2 * n_samples).astype(np.float32)
    nib = ((g[0::2] < 0) * 1 + (g[1::2] < 0) * 2 + (np.abs(g[0::2]) > 1) * 4 + (np.abs(g[1::2]) > 1) * 8).astype(np.uint8)
    packed = (nib[0::2] | (nib[1::2] << 4)).astype(np.uint8)
    pairs = np.empty(2 * n_samples, dtype=np.int8)
    pairs[0::4], pairs[1::4] = LUT_I[packed & 15], LUT_Q[packed & 15]
    pairs[2::4], pairs[3::4] = LUT_I[packed >> 4], LUT_Q[packed >> 4]
    return packed, pairs


def write_repeated(path, block, n_bytes):
    with open(path, "wb") as f:
        left = n_bytes
        while left > 0:
            m = min(left, block.size)
            f.write(block[:m].tobytes())
            left -= m


def settings_and_channels(epochs, file_type, n_ch=12):
    import bds_amd

    s = bds_amd.init_settings_b1c(samplingFreq=99.375e6, IF=14.58e6, msToProcess=epochs * 10, numberOfChannels=n_ch, pilotTRKflag=2,
                                  fileType=file_type)
    ch = [SimpleNamespace(PRN=p, acquiredFreq=s.IF + 100.0 * i, codePhase=float(1000 * i + 1 + (i & 1)), codeFreq=s.codeFreqBasis, status="T")
          for i, p in enumerate(range(1, n_ch + 1))]
    return s, ch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=1200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limits", default="0,256")
    ap.add_argument("--dir", default=os.environ.get("BDS_BENCH_TMP", tempfile.gettempdir()))
    ap.add_argument("--profile", type=int, choices=(2, 3), default=0)
    a = ap.parse_args()
    import bds_amd

    ctx = bds_amd.get_context(0)
    print(f"# library {os.environ.get('BDS_LIB_PATH', 'libbds_mi355x.so (in-tree release build)')}")
    packed, pairs = noise_block(BLOCK_EPOCHS * SPC)
    n = (a.epochs + 3) * SPC  # samples of the record (even)
    if a.profile:
        # one call from memory, warm-up included: every k_trk_correlate launch of the process is of this format
        reps = -(-n // (BLOCK_EPOCHS * SPC))
        x = np.tile(packed, reps)[: n // 2] if a.profile == 3 else np.tile(pairs, reps)[: 2 * n]
        s, ch = settings_and_channels(a.epochs, a.profile)
        bds_amd.tracking(x, ch, s.copy(msToProcess=100), mode="WB")
        res, _ = bds_amd.tracking(x, ch, s, mode="WB")
        print(f"fileType {a.profile}: {a.epochs} epochs from memory, total_ms {ctx.timing()['total_ms']:.2f}, "
              f"ms per epoch {ctx.timing()['total_ms'] / a.epochs:.4f}, completed {sorted({int(q.completed) for q in res})}, sha256 {digest(res)}")
        return
    paths = {}
    try:
        for ft, block, nb in ((2, pairs, 2 * n), (3, packed, n // 2)):
            fd, paths[ft] = tempfile.mkstemp(prefix=f"bds_packed_ft{ft}_", suffix=".bin", dir=a.dir)
            os.close(fd)
            write_repeated(paths[ft], block, nb)
        print(f"# 12 channels x {a.epochs} WB epochs, fs 99.375 MS/s; fileType 2 record {2 * n / 1e9:.3f} GB, fileType 3 record {n / 2 / 1e9:.3f} GB, in {a.dir}")
        out = {}
        for ft in (2, 3):
            s, ch = settings_and_channels(a.epochs, ft)
            bds_amd.tracking(paths[ft], ch, s.copy(msToProcess=100), mode="WB")  # warm-up: code tables, kernels, the file in the page cache
            for mib in [int(v) for v in a.limits.split(",")]:
                kw = {"resident_limit": mib << 20} if mib else {}
                wall, own = [], []
                for r in range(a.repeats):
                    t0 = time.perf_counter()
                    res, _ = bds_amd.tracking(paths[ft], ch, s, mode="WB", **kw)
                    wall.append(time.perf_counter() - t0)
                    own.append(ctx.timing()["total_ms"])
                    print(f"fileType {ft} limit {mib} MiB repeat {r}: wall {wall[-1]:.4f} s, total_ms {own[-1]:.2f}")
                info = ctx.track_stream_info()
                d = digest(res)
                out[(ft, mib)] = dict(wall=wall, own=own, loaded=ctx.track_loaded_bytes(), info=info, sha=d)
                print(f"fileType {ft} limit {mib} MiB: wall s median {np.median(wall):.4f} min {min(wall):.4f} max {max(wall):.4f} max-min {max(wall) - min(wall):.4f};  "
                      f"total_ms median {np.median(own):.2f} min {min(own):.2f} max {max(own):.2f} max-min {max(own) - min(own):.2f};  "
                      f"completed {sorted({int(q.completed) for q in res})}  loaded {ctx.track_loaded_bytes()} bytes  {info}")
                print(f"fileType {ft} limit {mib} MiB: results sha256 {d}")
        for mib in [int(v) for v in a.limits.split(",")]:
            i, p = out[(2, mib)], out[(3, mib)]
            print(f"limit {mib} MiB: results {'bit-identical' if i['sha'] == p['sha'] else 'DIFFER'};  loaded bytes 3 / 2 = {p['loaded'] / i['loaded']:.4f};  "
                  f"wall median 3 / 2 = {np.median(p['wall']) / np.median(i['wall']):.3f};  total_ms median 3 / 2 = {np.median(p['own']) / np.median(i['own']):.3f}")
        if (2, 0) in out:
            i, p = out[(2, 0)], out[(3, 0)]
            bound = np.median(i["own"]) * 1.05 + (max(i["own"]) - min(i["own"]))
            print(f"decode cost, one window: fileType 3 total_ms median {np.median(p['own']):.2f} against fileType 2 median x 1.05 + its max-min = {bound:.2f}: "
                  f"{'within' if np.median(p['own']) <= bound else 'SLOWER than'} the bound")
    finally:
        for q in paths.values():
            if os.path.exists(q):
                os.remove(q)


if __name__ == "__main__":
    main()
