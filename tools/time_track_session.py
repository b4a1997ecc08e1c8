#!/usr/bin/env python3
"""What a tracking session costs, on cfg4's 12 wide-band channels (99.375 MS/s, bench.track_record) over --epochs epochs:
    python tools/time_track_session.py [--parent-lib PATH] [--epochs 200] [--repeats 5] [--out profiles/r11_track_session.txt]
Same box, same run, --repeats wall times each (record in host memory, one warm-up first) of
    one-shot   one bds_track_mem call on this build
    parent     the same call on a build of the parent commit (--parent-lib: its libbds_mi355x.so; a child process that loads it
               through BDS_LIB_PATH, as tools/time_acq.py is run once per library)
    advance-N  a session as one advance(N)              (the open and the close are timed apart)
    advance-1  a session as N x advance(1)
and from them
    the one condition      one-shot (median) - parent (median) <= parent's own max - min over its repeats: the split of
                           do_track must cost nothing
    per-advance overhead   (advance-1 - advance-N) / N, reported without a threshold
The session's arrays are checked against the one-shot call's (bit-equal) before anything is timed."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def case(epochs):
    import bds_amd
    import bench

    base = bds_amd.init_settings_b1c(samplingFreq=99.375e6, IF=14.58e6, acqSatelliteList=list(range(1, 64)), acqCohT=10, pilotACQflag=1)
    s, x, ch, mode, _ = bench.track_record("b1c", base, epochs=epochs)
    return s, x, ch, mode


def time_one_shot(s, x, ch, mode, repeats):
    import bds_amd

    bds_amd.tracking(x, ch, s, mode=mode)  # warm-up: code tables, first allocation
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        res, _ = bds_amd.tracking(x, ch, s, mode=mode)
        out.append(time.perf_counter() - t0)
    assert all(r.completed == len(r.I_P) for r in res)
    return out, res


def time_session(s, x, ch, mode, epochs, piece, repeats, want):
    import bds_amd

    walls, opens = [], []
    for rep in range(repeats + 1):  # (the first is the warm-up)
        t0 = time.perf_counter()
        t = bds_amd.TrackSession(x, ch, s, mode=mode)
        t1 = time.perf_counter()
        calls = [t.advance(piece) for _ in range(epochs // piece)]
        t2 = time.perf_counter()
        t.close()
        t3 = time.perf_counter()
        if rep == 0:
            for c, w in enumerate(want):
                for f in ("I_P", "Q_P", "carrFreq", "codeFreq", "absoluteSample", "DataCNo", "B1C_CNo"):
                    np.testing.assert_array_equal(np.concatenate([call[c].__dict__[f] for call in calls]), getattr(w, f), err_msg=f)
            continue
        walls.append(t2 - t1)
        opens.append((t1 - t0) + (t3 - t2))
    return walls, opens


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "all": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one-shot-only", action="store_true", help=argparse.SUPPRESS)  # the child process of --parent-lib
    a = ap.parse_args()
    s, x, ch, mode = case(a.epochs)
    one, want = time_one_shot(s, x, ch, mode, a.repeats)
    if a.one_shot_only:
        print("ONE_SHOT " + json.dumps(one))
        return
    res = {"one-shot": stats(one)}
    if a.parent_lib:
        env = dict(os.environ, BDS_LIB_PATH=os.path.abspath(a.parent_lib))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one-shot-only", "--epochs", str(a.epochs), "--repeats", str(a.repeats)],
                             env=env, check=True, capture_output=True, text=True).stdout
        res["parent"] = stats(json.loads([ln for ln in out.splitlines() if ln.startswith("ONE_SHOT ")][-1][9:]))
    w, o = time_session(s, x, ch, mode, a.epochs, a.epochs, a.repeats, want)
    res[f"advance-{a.epochs}"], res["open+close (advance-N runs)"] = stats(w), stats(o)
    w1, _ = time_session(s, x, ch, mode, a.epochs, 1, a.repeats, want)
    res["advance-1"] = stats(w1)
    lines = [f"tracking sessions: 12 wide-band channels, {a.epochs} epochs of 10 ms at 99.375 MS/s, record in host memory, {a.repeats} repeats, seconds"]
    for k, v in res.items():
        lines.append(f"  {k:30s} median {v['median']:.4f}  min {v['min']:.4f}  max {v['max']:.4f}   {' '.join('%.4f' % t for t in v['all'])}")
    over = (res["advance-1"]["median"] - res[f"advance-{a.epochs}"]["median"]) / a.epochs
    lines.append(f"  per-advance overhead (advance-1 - advance-{a.epochs}) / {a.epochs} = {over * 1e6:.1f} us")
    if "parent" in res:
        diff, spread = res["one-shot"]["median"] - res["parent"]["median"], res["parent"]["max"] - res["parent"]["min"]
        lines.append(f"  one-shot - parent = {diff * 1e3:+.2f} ms, parent's max - min = {spread * 1e3:.2f} ms: "
                     + ("the split costs nothing" if diff <= spread else "THE ONE-SHOT CALL IS SLOWER THAN THE PARENT'S"))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
