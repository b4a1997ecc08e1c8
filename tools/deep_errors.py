#!/usr/bin/env python3
"""Worst error of the weak-signal acquisition's accumulated surfaces on one MI355X against the NumPy float64 model of
tests/deep_cases.py, on the scenes of tests/test_deep_gpu.py and on the forced column plans of tests/test_deep_plans_gpu.py: every
value of every row through bds_acq_deep_row, as a fraction of the tolerance 2e-5 sum_k (max m_k)^2 of its PRN; and deepMetric
against the bound that tolerance propagates to.

  python tools/deep_errors.py [--out profiles/deep_errors.txt]"""
import argparse
import contextlib
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("BDS_LIB_PATH", os.path.join(ROOT, "bds-3-b1c-b2a-sdr-receiver_amd", "libbds_mi355x_hooks.so"))  # forced plans: test-hooks build only


@contextlib.contextmanager
def stderr_text():
    """What the library writes to file descriptor 2 inside the block; the function it yields returns the text afterwards."""
    sys.stderr.flush()
    saved, box = os.dup(2), []
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            yield lambda: box[0]
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            f.seek(0)
            box.append(f.read().decode(errors="replace"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bds_amd
    import deep_cases as dc

    ctx = bds_amd.get_context(0)
    lines = [f"bds_acq_deep on {ctx.device_name()} against the float64 model (tests/deep_cases.py)",
             "surface: worst |S_gpu - S_model| over all D x N values / tolerance (2e-5 sum_k (max m_k)^2); deepMetric: |error| / its bound", ""]
    for name in sorted(dc.GPU_SCENES):
        s, _, k = dc.GPU_SCENES[name]()
        err = dc.surface_errors(name)
        got = dc.run_scene(name, keep_surface=False)
        for prn, r in dc.scene_model(name).items():
            dm = abs(got.deepMetric[prn - 1] - r.deepMetric)
            lines.append(f"{name:18s} K = {k:2d} PRN {prn:2d}  surface {err[prn]:.3e}   deepMetric {r.deepMetric:8.3f} error {dm:.2e} = {dm / dc.deep_metric_bound(r):.3e} of its bound")
    for prn, e in dc.surface_errors("drift_b2a", compensate=False).items():
        lines.append(f"{'drift_b2a':18s} K = 16 PRN {prn:2d}  surface {e:.3e}   (compensate = 0)")
    lines += ["", "forced column plans (BDS_ACQ_FORCE_L1L2 of the test-hooks build; tests/test_deep_plans_gpu.py), the plan as the library's plan line names it"]
    forced = [("plans_b2a", p) for p in sorted(dc.PLANS_B2A, key=lambda p: int(p.split("x")[0]))]
    forced += [(name, p) for name in ("plans_b1c", "plans_b1c_nopilot") for p in ("1024x270", "1280x324")]
    forced += [("chunks_b2a", "1280x324")]  # 201 bins in chunks of 161 and 40
    for name, plan in forced:
        with dc.verbose_plans(ctx), stderr_text() as err:
            e = dc.surface_errors(name, plan=plan)
        _, (_, l1, l2) = dc.plans_that_ran(err())  # (the plan that wrote the stale surfaces, the plan under test)
        assert f"{l1}x{l2}" == plan, (plan, l1, l2)
        lines += [f"{name:18s} plan {l1:4d} x {l2:4d} PRN {prn:2d}  surface {v:.3e}" for prn, v in e.items()]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
