"""The chunk list of the N-point row pass (csrc/bds_acq.hip, rows_chunk_plan) through the hooks library, no GPU: for every launch pair
of 1..32 PRNs x 201 cells on 512 resident workgroups the chunks partition each PRN's cells, none crosses a PRN, sizes never increase
along the list, and the makespan -- by this file's own simulation -- is never above that of the uniform chunks the library took before
(67 cells for these shapes: the largest divisor of 201 that gives 32 waves of workgroups or, failing that, stays at or above 32 cells).

The model of the simulation is the one the planner is specified against: greedy assignment in block order onto the slots; a launch
has 27 x 12 workgroups per chunk, of which the 6 of the last row pair with an odd k2 return at once (no time), the others run for
(cells of the chunk + SETUP) cell-times.  SETUP is checked at 0 and at one cell as well as at the planner's own 3 / 8: the list may not
owe its advantage to the set-up figure."""
import ctypes as C
import heapq

import pytest

from bds_amd import native

D, SLOTS = 201, 512
WGS_PER_CHUNK, IDLE_PER_CHUNK = 27 * 12, 6
NPS = list(range(1, 33))


def plan(np_, d=D, slots=SLOTS):
    lib = native.lib()
    assert native.has_test_hooks(), "the planner is exported by the test-hooks build only"
    f = lib.bds_test_rows_chunks
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]
    n = f(np_, d, slots, None, 0)
    assert 0 < n <= np_ * d
    buf = (C.c_int * (2 * n))()
    assert f(np_, d, slots, buf, n) == n
    return [(buf[2 * i], buf[2 * i + 1]) for i in range(n)]


_plans = {}


def cached_plan(np_):
    if np_ not in _plans:
        _plans[np_] = plan(np_)
    return _plans[np_]


def uniform_gc(np_, d=D):
    """The rule of the uniform path (rows_uniform_gc with BDS_ACQ_LIST_GC unset)."""
    gc = d
    for dv in range(1, d + 1):
        if d % dv:
            continue
        if d // dv < 32 and dv > 1:
            break
        gc = d // dv
        if WGS_PER_CHUNK * np_ * dv >= 32 * 512:
            break
    return gc


def makespan(sizes, setup8, slots=SLOTS):
    """In eighths of a cell-time."""
    free_at = [0] * slots
    end = 0
    for sz in sizes:
        d = 8 * sz + setup8
        for _ in range(WGS_PER_CHUNK - IDLE_PER_CHUNK):
            t = free_at[0] + d
            heapq.heapreplace(free_at, t)
            end = max(end, t)
    return end


def test_uniform_rule_of_these_shapes():
    assert {uniform_gc(n) for n in NPS} == {67} and uniform_gc(51) == 201


@pytest.mark.parametrize("np_", NPS)
def test_list_is_a_partition_in_non_increasing_sizes(np_):
    chunks = cached_plan(np_)
    seen = [0] * (np_ * D)
    for first, count in chunks:
        assert count >= 1 and 0 <= first and first + count <= np_ * D
        assert first // D == (first + count - 1) // D, "a chunk crosses a PRN"
        for c in range(first, first + count):
            seen[c] += 1
    assert seen == [1] * (np_ * D)  # every cell of every PRN exactly once
    sizes = [c for _, c in chunks]
    assert all(a >= b for a, b in zip(sizes, sizes[1:])), "sizes increase along the list"


@pytest.mark.parametrize("np_", NPS)
def test_makespan_not_above_the_uniform_choice(np_):
    sizes = [c for _, c in cached_plan(np_)]
    gc = uniform_gc(np_)
    uniform = [gc] * (np_ * D // gc)
    for setup8 in (0, 3, 8):
        assert makespan(sizes, setup8) <= makespan(uniform, setup8), (np_, setup8)


def test_cfg3_pairs_come_close_to_the_ideal():
    """13 and 11 PRNs (what a cfg3 call launches): within 1 % of cells x working workgroups / slots; uniform 67 is 3.8 and 3.0 % above."""
    for np_ in (13, 11):
        ideal8 = 8 * np_ * D * (WGS_PER_CHUNK - IDLE_PER_CHUNK) / SLOTS
        assert makespan([c for _, c in cached_plan(np_)], 3) <= 1.01 * ideal8
        assert min(c for _, c in cached_plan(np_)) < 32  # small chunks close the launch


def test_planner_is_deterministic():
    for np_ in (1, 7, 13, 32):
        assert plan(np_) == cached_plan(np_)


def test_other_shapes_and_arguments():
    for np_, d, slots in ((1, 1, 512), (3, 7, 16), (2, 201, 608), (5, 64, 512)):
        chunks = plan(np_, d, slots)
        assert sorted(c for f, n in chunks for c in range(f, f + n)) == list(range(np_ * d))
        assert all(f // d == (f + n - 1) // d for f, n in chunks)
    f = native.lib().bds_test_rows_chunks
    assert f(0, 201, 512, None, 0) < 0 and f(1, 0, 512, None, 0) < 0 and f(1, 201, 0, None, 0) < 0
