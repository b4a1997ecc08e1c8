"""The column pass of the weak-signal acquisition (k_cols_deep, csrc/bds_acq_deep.h) on the plans it was written for, at small N.

The scenes of tests/test_deep_gpu.py all plan a 40-point column pass: one wave per workgroup, T = 16, whole tiles, a tile count
that is a multiple of 8.  The full rates plan 256- to 1024-point columns (4 to 16 waves, up to 139 648 B of LDS).  Those plans are
forced here on 12 MS/s / 5 MS/s records (BDS_ACQ_FORCE_L1L2 of the test-hooks build) -- every one within the planner's own limits,
so a plan it could pick for some record -- and ALL D x N surface values of every PRN are held to the float64 model at the
tolerance of test_deep_gpu.test_surface_values.  The model does not depend on the plan: one cached model per scene serves them all.
The surface is never zeroed (block 0 stores), so a tile the pass skips keeps what the buffer held and a doubled one has twice the
value; tests/test_deep_cases.py shows that a missing or doubled tile is more than 100 tolerances away, and every run here writes
into surfaces that hold the values of another record (deep_cases.run_scene_on_stale_surfaces).

What each plan reaches (T, tiles, columns of the last tile: deep_cases.PLANS_B2A, from deep_plan's rules):
  9 x 4096     the planner's choice: one wave, whole tiles
  8 x 4500     L = need + 1; 282 tiles (not a multiple of 8: xcd_remap's uneven runs), the last of 4 columns; 320-thread rows with
               radix-5 and radix-3 stages
  256 x 144    4 waves, 9 tiles: the column plan of B2a at 99.375 MS/s
  375 x 96     448 threads (7 waves); columns of radix 5 and 3 only
  512 x 135    8 waves, last tile 7 columns: the column plan of B1C at 53 MS/s
  768 x 200    832 threads, 13 tiles, last tile 8 columns
  1024 x 270   1024 threads, 139 648 B of LDS, 17 tiles, last tile 14 columns; L = 11.5 N: most outputs fail `lag < N`
  1280 x 324   T = 8 (logT = 3), 704 threads, 41 tiles, last tile 4 columns
Measured worst ratios: profiles/deep_errors.txt."""
import pytest

import deep_cases as dc

pytestmark = pytest.mark.gpu


def _pair(plan):
    return tuple(int(v) for v in plan.split("x"))


def _surface_on_plan(ctx, capfd, name, plan, planner):
    """The scene's surfaces on a forced plan (None: the planner's, which is `planner`) against the model.  The plan lines must name
    the plan that wrote the stale surfaces and then the plan under test: a forced plan the library rejects falls back silently."""
    s, _, _ = dc.GPU_SCENES[name]()
    _, x_len, n, _ = dc.sizes(s)
    need = n + x_len - 1
    ran = _pair(plan) if plan else planner
    with dc.verbose_plans(ctx):
        capfd.readouterr()
        errors = dc.surface_errors(name, plan=plan)
        plans = dc.plans_that_ran(capfd.readouterr().err)
    assert plans == [(need,) + (planner if plan else _pair(dc.STALE_PLAN)), (need,) + ran], (plan, plans)
    for prn, ratio in errors.items():
        print(f"\ndeep_errors: {name} plan {ran[0]} x {ran[1]} PRN {prn} worst |error| / tolerance = {ratio:.3e}")
        assert ratio <= 1.0, (name, plan, prn, ratio)


@pytest.mark.parametrize("plan", [None] + sorted(dc.PLANS_B2A, key=lambda p: _pair(p)[0]))
def test_surface_values_b2a(ctx, capfd, plan):
    """Two components (NCOMP = 2), 2 PRNs x 9 bins x 24000 lags, K = 3."""
    if plan:
        (l1, l2), (t, tiles, last) = _pair(plan), dc.PLANS_B2A[plan]
        assert l1 * l2 >= 35999 and tiles == -(-l2 // t) and last == l2 - (tiles - 1) * t  # (the table above)
    _surface_on_plan(ctx, capfd, "plans_b2a", plan, (9, 4096))


@pytest.mark.parametrize("plan", [None, "1024x270", "1280x324"])
@pytest.mark.parametrize("name", ["plans_b1c", "plans_b1c_nopilot"])
def test_surface_values_b1c(ctx, capfd, name, plan):
    """B1C with acqCohT = 2 (N = 60000, need 69999): both instantiations, the weighted pair and the single component, on the planner's
    12 x 6144 and on the 16-wave and the T = 8 plans."""
    _surface_on_plan(ctx, capfd, name, plan, (12, 6144))


def test_forced_plan_does_not_outlive_its_test(ctx, capfd):
    """After a run on a forced plan the variable is gone and the next run plans for itself."""
    import os

    with dc.verbose_plans(ctx):
        dc.run_scene_on_stale_surfaces("plans_b2a", "256x144")
    assert "BDS_ACQ_FORCE_L1L2" not in os.environ
    with dc.verbose_plans(ctx):
        capfd.readouterr()
        dc.run_scene("plans_b2a", keep_surface=False)
        assert dc.plans_that_ran(capfd.readouterr().err) == [(35999, 9, 4096)]
