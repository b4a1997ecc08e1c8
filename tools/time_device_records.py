#!/usr/bin/env python3
"""What the host round trip of an IF record costs, and what the *_dev entries save -> profiles/r14_device_records_<box>.txt.

Tracking.  The record has cfg4's size: 12 B1C satellites (cfg4's Dopplers, code Doppler on, 47 dB-Hz) at 99.375 MS/s, 12 wide-band
channels, --epochs ten-millisecond epochs (default 3 600: 3.58 GB of int8), 256 MiB of it resident (a session's default).  In one
process, on one box, --repeats times each after one warm-up:
    (a) file     write_if(path) (bds_synth_file) + TrackSession(path): the record generated on the card, copied to the host,
                 written, read back by the loader thread and tracked
    (b) host     a feed session fed from PINNED host memory holding the same bytes, --chunk bytes per feed
    (c) device   the record generated with bds_synth_dev in pieces of --chunk bytes into one device buffer and fed with
                 bds_track_feed_dev: it never leaves HBM
Reported: wall time, the time inside advance() (the epoch loop, which in (a) also waits for the loader), the time inside feed()
and its bytes per second, and for (c) the time inside the generator.  The three runs' Pilot_I_P / carrFreq arrays are compared
(the bytes are the same, so the results are: bit-equal) before anything is reported.

Acquisition.  acq_load of a cfg3-size block (B1C at 99.375 MS/s, 4 code periods = 3.975 MB of int8) from pageable host memory,
pinned host memory and device memory, wall time per call.

    python tools/time_device_records.py [--out profiles/r14_device_records_<box>.txt] [--epochs 3600] [--repeats 3] [--chunk 67108864] [--tmp DIR]
"""
import argparse
import os
import socket
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bds_amd  # noqa: E402
from bds_amd import synth  # noqa: E402

ADVANCE = 1000  # epochs asked of one advance()
SEED = 14


def case(epochs):
    s = bds_amd.init_settings_b1c(samplingFreq=99.375e6, IF=14.58e6, acqSatelliteList=list(range(1, 64)), acqCohT=10, pilotACQflag=1,
                                  msToProcess=epochs * 10, numberOfChannels=12, pilotTRKflag=2)
    spc = int(np.floor(s.samplingFreq / (s.codeFreqBasis / s.codeLength) + 0.5))
    rng = np.random.default_rng(1)
    dopplers = [-1500, -1000, -750, -500, -250, -100, 100, 250, 500, 750, 1000, 1500]
    sats = [synth.Sat(p, float(d), float(rng.uniform(0.2, 0.8)) * spc, float(rng.uniform(0, 2 * np.pi)), 47.0) for p, d in zip(range(1, 13), dopplers)]
    ch = []
    for sat in sats:
        cf = s.IF + round(sat.doppler / 25) * 25
        ch.append(SimpleNamespace(PRN=sat.prn, acquiredFreq=float(cf), codePhase=float(int(np.ceil(sat.delay)) + 1),
                                  codeFreq=float(s.codeFreqBasis - (cf - s.IF) / s.carrFreqBasis * s.codeFreqBasis), status="T"))
    n = (epochs + 3) * spc
    return s, sats, ch, n - n % 32, spc


def drain(t, keep, clock):
    """advance until nothing runs any more; the time goes to clock["advance"], the arrays to keep"""
    while True:
        t0 = time.perf_counter()
        r = t.advance(ADVANCE)
        clock["advance"] += time.perf_counter() - t0
        if not t.last_k:
            return
        keep.append([(q.Pilot_I_P, q.carrFreq, q.completed) for q in r])


def joined(keep):
    return [(np.concatenate([call[c][0] for call in keep]), np.concatenate([call[c][1] for call in keep]), sum(call[c][2] for call in keep))
            for c in range(len(keep[0]))]


def run_file(s, sats, ch, n, path, epochs):
    clock = {"advance": 0.0, "feed": 0.0, "generate": 0.0}
    keep = []
    t0 = time.perf_counter()
    synth.write_if(path, s, sats, n, seed=SEED)
    clock["generate"] = time.perf_counter() - t0
    with bds_amd.TrackSession(path, ch, s, mode="WB") as t:
        left = epochs
        while left > 0:
            t1 = time.perf_counter()
            r = t.advance(min(ADVANCE, left))
            clock["advance"] += time.perf_counter() - t1
            if not t.last_k:
                break
            left -= t.last_k
            keep.append([(q.Pilot_I_P, q.carrFreq, q.completed) for q in r])
    clock["wall"] = time.perf_counter() - t0
    return clock, joined(keep)


def feed_run(s, ch, pieces, epochs):
    """A feed session over pieces(): an iterator of (array, is_last) whose production time it books under "generate"."""
    clock = {"advance": 0.0, "feed": 0.0, "generate": 0.0}
    keep = []
    t0 = time.perf_counter()
    with bds_amd.TrackSession(None, ch, s, origin=0, mode="WB") as t:
        it = iter(pieces)
        while True:
            t1 = time.perf_counter()
            nxt = next(it, None)
            clock["generate"] += time.perf_counter() - t1
            if nxt is None:
                break
            piece, is_last = nxt
            while True:
                t1 = time.perf_counter()
                took = t.feed(piece, last=is_last)
                clock["feed"] += time.perf_counter() - t1
                t1 = time.perf_counter()
                r = t.advance(ADVANCE)
                clock["advance"] += time.perf_counter() - t1
                if t.last_k:
                    keep.append([(q.Pilot_I_P, q.carrFreq, q.completed) for q in r])
                assert took or t.last_k
                piece = piece[took:]
                if len(piece) == 0:
                    break
        drain(t, keep, clock)
    clock["wall"] = time.perf_counter() - t0
    got = joined(keep)
    return clock, [(a[:epochs], b[:epochs], min(c, epochs)) for a, b, c in got]


def fmt_row(name, rows, n_bytes):
    def mm(k):
        v = [r[k] for r in rows]
        return "%7.3f .. %-7.3f" % (min(v), max(v))
    feed = min(r["feed"] for r in rows)
    return "%-10s %s %s %s %s %s" % (name, mm("wall"), mm("advance"), mm("feed"), mm("generate"), "%8.1f" % (n_bytes / feed / 1e9) if feed > 0 else "       -")


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_device_records_%s.txt" % socket.gethostname()))
    ap.add_argument("--epochs", type=int, default=3600)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=64 << 20)
    ap.add_argument("--tmp", default=tempfile.gettempdir())
    a = ap.parse_args()
    ctx = bds_amd.get_context(0)
    s, sats, ch, n, spc = case(a.epochs)
    path = os.path.join(a.tmp, "bds_time_device_records_%d.bin" % os.getpid())
    rows = {"file": [], "host": [], "device": []}
    try:
        # (b)'s bytes: the file of a first (a) run, read into pinned memory (not timed)
        _, want = run_file(s, sats, ch, n, path, a.epochs)
        pinned = torch.empty(n, dtype=torch.int8, pin_memory=True)
        host = pinned.numpy()
        with open(path, "rb") as f:
            assert f.readinto(memoryview(host).cast("B")) == n
        d_buf = torch.empty(a.chunk, dtype=torch.int8, device="cuda:0")

        def host_pieces():
            for o in range(0, n, a.chunk):
                yield host[o:o + a.chunk], o + a.chunk >= n

        def device_pieces():
            for o in range(0, n, a.chunk):
                m = min(a.chunk, n - o)
                ctx.synth_dev(s, sats, o, m, 1, d_buf[:m], seed=SEED)
                yield d_buf[:m], o + m >= n

        for rep in range(a.repeats + 1):  # (the first is the warm-up, and the check)
            for name, run in (("file", lambda: run_file(s, sats, ch, n, path, a.epochs)), ("host", lambda: feed_run(s, ch, host_pieces(), a.epochs)),
                              ("device", lambda: feed_run(s, ch, device_pieces(), a.epochs))):
                clock, got = run()
                if rep == 0:
                    for c, (w, g) in enumerate(zip(want, got)):
                        assert w[2] == g[2] == a.epochs, (name, c, w[2], g[2])
                        np.testing.assert_array_equal(g[0], w[0], err_msg="%s channel %d Pilot_I_P" % (name, c))
                        np.testing.assert_array_equal(g[1], w[1], err_msg="%s channel %d carrFreq" % (name, c))
                else:
                    rows[name].append(clock)
        locked = sum(bool(abs(w[1][-1] - (s.IF + sat.doppler)) < 5.0) for w, sat in zip(want, sats))  # carrFreq within 5 Hz of the truth at the end
    finally:
        if os.path.exists(path):
            os.remove(path)
    lines = ["# tools/time_device_records.py on %s, box %s" % (ctx.device_name(), socket.gethostname()),
             "# tracking: %d B1C satellites at %.3f MS/s (code Doppler on), 12 wide-band channels, %d epochs of 10 ms, record of %d samples (%.2f GB int8)," % (
                 len(sats), s.samplingFreq / 1e6, a.epochs, n, n / 1e9),
             "# 256 MiB resident, feeds and generator pieces of %d bytes, advance(%d); seconds, min .. max of %d runs after one warm-up run" % (a.chunk, ADVANCE, a.repeats),
             "# (a) file: write_if + TrackSession(path) -- `generate` is write_if (generator, copy to the host, write), `advance` includes waiting for the loader thread",
             "# (b) host: feed session from pinned host memory   (c) device: bds_synth_dev pieces + bds_track_feed_dev -- `generate` is the generator's calls",
             "# all three runs: %d epochs on every channel, Pilot_I_P and carrFreq bit-equal between them; %d of 12 channels end within 5 Hz of their carrier" % (a.epochs, locked),
             "source     wall s             in advance() s     in feed() s        generate s         feed GB/s"]
    for name in ("file", "host", "device"):
        lines.append(fmt_row(name, rows[name], n))
    w = {k: min(r["wall"] for r in rows[k]) for k in rows}
    lines.append("(c) against (a): %.2f x the wall time (%.3f s of %.3f s); (c) against (b): %.2f x (%.3f s of %.3f s)" % (
        w["device"] / w["file"], w["device"], w["file"], w["device"] / w["host"], w["device"], w["host"]))
    # acquisition: acq_load alone
    sa = s
    block_d = synth.make_if_device(sa, sats, 4 * spc, seed=SEED, out="torch")
    block_h = block_d.cpu().numpy()
    block_p = torch.empty(block_h.size, dtype=torch.int8, pin_memory=True)
    block_p.copy_(torch.from_numpy(block_h))
    res = {}
    for name, src in (("pageable host", block_h), ("pinned host", block_p.numpy()), ("device", block_d)):
        ctx.acq_load(sa, src)
        v = []
        for _ in range(max(a.repeats, 5)):
            t0 = time.perf_counter()
            ctx.acq_load(sa, src)
            v.append(time.perf_counter() - t0)
        res[name] = v
    lines.append("# acquisition: acq_load of %d int8 samples (%.2f MB, cfg3's block), wall ms per call, min .. max of %d" % (block_h.size, block_h.size / 1e6, max(a.repeats, 5)))
    for name, v in res.items():
        lines.append("acq_load   %-14s %7.3f .. %-7.3f" % (name, min(v) * 1e3, max(v) * 1e3))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
