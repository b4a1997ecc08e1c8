"""Placement and LDS layout of the N-point row pass k_pfa_rows<2> (csrc/bds_acq_pfa.h) through the hooks library, no GPU.  Both come from
the functions the kernel itself calls (rows_pos / rows_place, rows_lds_index); this file holds the model they are specified against.

Placement.  A chunk of cells is 328 = 8 x 41 workgroups; workgroup l of a chunk is taken to sit behind L2 number l % 8 (workgroups are
dealt round-robin over the 8 XCDs, and 328 % 8 = 0 keeps the label the same in every chunk).  The 318 working (mp, k2) -- 26 row pairs
x 12 k2, and the last pair's single row 52 as 6 workgroups of an even k2 and its successor -- appear exactly once, 10 positions are idle,
and no label holds more than 40 working workgroups.  One cell later a workgroup reads, for each of its two rows (k1, k2), the signal row
that the owner of row (k1 - 1 mod 53, k2 - 1 mod 12) reads now: the share of these 636 partner rows whose owner has the workgroup's own
label is 530 / 636 = 5 / 6, and at least 0.75.

LDS.  Bank rule of the kernel's comments: 64 banks of 4 bytes; a ds_read_b64 is served per 32-lane half, a ds_write_b64 per 16-lane
group; two lanes of such a group conflict when they touch different 8-byte elements whose indices agree modulo 32.  A row is 125 live
threads j = 32 wave + lane (the row's partner sits in the other halves of the same four waves, in a region of its own whose offset is a
multiple of 32 elements), so a half is j = 32 w .. 32 w + 31 and a write group j = 16 g .. 16 g + 15.  Every access of the three stages
is enumerated."""
import ctypes as C

import numpy as np
import pytest

from bds_amd import native

MP, K1, K2, K3 = 27, 53, 12, 3125
WGS, WORKING, XCDS = 328, 318, 8
LIVE = 125


@pytest.fixture(scope="module")
def lib():
    L = native.lib()
    assert native.has_test_hooks(), "the placement is exported by the test-hooks build only"
    L.bds_test_rows_place.restype = C.c_int
    L.bds_test_rows_place.argtypes = [C.POINTER(C.c_int), C.c_int]
    L.bds_test_rows_lds_index.restype = C.c_int
    L.bds_test_rows_lds_index.argtypes = [C.c_int]
    return L


@pytest.fixture(scope="module")
def table(lib):
    """[(position, 12 mp + k2 or -1)] per workgroup l of a chunk."""
    n = lib.bds_test_rows_place(None, 0)
    assert n == WGS and WGS % XCDS == 0  # blockIdx.x = WGS chunk + l: l % 8 is blockIdx.x % 8 in every chunk, chunk = blockIdx.x // WGS
    buf = (C.c_int * (2 * n))()
    assert lib.bds_test_rows_place(buf, n) == n
    assert lib.bds_test_rows_place(None, 4) < 0
    return [(buf[2 * l], buf[2 * l + 1]) for l in range(n)]


@pytest.fixture(scope="module")
def lds(lib):
    idx = np.array([lib.bds_test_rows_lds_index(e) for e in range(K3)])
    assert lib.bds_test_rows_lds_index(-1) < 0 and lib.bds_test_rows_lds_index(K3) < 0
    return idx


def working_set():
    return {12 * mp + k2 for mp in range(MP - 1) for k2 in range(K2)} | {12 * (MP - 1) + k2 for k2 in range(0, K2, 2)}


def test_positions_are_a_bijection_in_bands(table):
    pos = [p for p, _ in table]
    assert sorted(pos) == list(range(WGS))
    for l, p in enumerate(pos):
        assert p // (WGS // XCDS) == l % XCDS  # a label is a band of consecutive positions


def test_every_working_pair_once_and_ten_idle(table):
    placed = [rp for _, rp in table if rp >= 0]
    assert len(placed) == WORKING and set(placed) == working_set() and len(working_set()) == WORKING
    assert sum(rp < 0 for _, rp in table) == WGS - WORKING == 10
    by_pos = dict(table)
    order = [by_pos[p] for p in range(WGS) if by_pos[p] >= 0]
    assert order == sorted(order)  # along the positions the workgroups keep the (mp, k2) order: a band is consecutive pairs
    per_label = [sum(1 for l, (_, rp) in enumerate(table) if rp >= 0 and l % XCDS == x) for x in range(XCDS)]
    print("\nworking workgroups per label:", per_label)
    assert max(per_label) == -(-WORKING // XCDS) == 40 and min(per_label) == 39


def owner(k1, k2):
    """The workgroup (as 12 mp + k2) that transforms row (k1, k2)."""
    return 12 * (k1 // 2) + k2 if k1 < K1 - 1 else 12 * (MP - 1) + (k2 & ~1)


def test_partner_share(table):
    label = {rp: l % XCDS for l, (_, rp) in enumerate(table) if rp >= 0}
    same = total = 0
    rows_seen = set()
    for rp, lb in sorted(label.items()):
        mp, k2 = divmod(rp, 12)
        rows = [(2 * mp, k2), (2 * mp + 1, k2)] if mp < MP - 1 else [(K1 - 1, k2), (K1 - 1, k2 + 1)]
        hits = []
        for k1, kk in rows:
            assert owner(k1, kk) == rp
            rows_seen.add((k1, kk))
            hits.append(label[owner((k1 - 1) % K1, (kk - 1) % K2)] == lb)
        same += sum(hits)
        total += 2
        if not all(hits):
            print(f"(mp {mp}, k2 {k2}) label {lb}: partner of its low row {'same' if hits[0] else 'other'}, of its high row {'same' if hits[1] else 'other'}")
    assert rows_seen == {(k1, k2) for k1 in range(K1) for k2 in range(K2)} and total == 2 * WORKING
    print(f"partner rows behind the same label: {same} of {total} = {same / total:.4f}")
    assert (same, total) == (530, 636)  # 5 / 6
    assert same / total >= 0.75


# ---- LDS ------------------------------------------------------------------------------------------------------------------------
def stage_accesses():
    """(name, group size, [element e[j] for the live threads j = 0..124]) for every LDS instruction of a row, in the kernel's terms."""
    j = np.arange(LIVE)
    si, spg = j // 5, j % 5
    out = []
    for p in range(25):  # stage 1 writes a[j][p] at 25 j + p
        out.append((f"stage 1 write p {p}", 16, 25 * j + p))
    for c5 in range(5):  # stage 2: five reads and five in-place writes at 625 r + 25 i + 5 pg + c5
        for r in range(5):
            out.append((f"stage 2 read c5 {c5} r {r}", 32, 625 * r + 25 * si + 5 * spg + c5))
        for u in range(5):
            out.append((f"stage 2 write c5 {c5} u {u}", 16, 625 * u + 25 * si + 5 * spg + c5))
    for i in range(25):  # stage 3 reads b[p][i][u] at 625 u + 25 i + p, thread p + 25 u
        out.append((f"stage 3 read i {i}", 32, 625 * (j // 25) + 25 * i + j % 25))
    return out


def conflicts(elems_idx, group):
    """Lanes beyond the first on a bank, summed over the groups of `group` lanes of the four waves (a row's lanes of wave w: j = 32 w ..)."""
    extra = 0
    for g0 in range(0, 128, group):
        lanes = elems_idx[g0:min(g0 + group, LIVE)]
        by_bank = {}
        for a in lanes:
            by_bank.setdefault(int(a) % 32, set()).add(int(a))
        extra += sum(len(v) - 1 for v in by_bank.values())
    return extra


def test_index_function(lds):
    assert np.array_equal(lds, np.arange(K3) + 8 * (np.arange(K3) // 625))
    assert len(set(lds.tolist())) == K3 and lds.max() < 3168


def test_no_bank_conflicts_in_any_stage(lds):
    acc = stage_accesses()
    assert len(acc) == 25 + 5 * 10 + 25
    bad = [(name, c) for name, group, e in acc for c in [conflicts(lds[e], group)] if c]
    assert not bad, bad[:8]
    # the model sees the layout this replaces: 625 u + 25 i + p unpadded is 2-way in each of the 25 stage-3 reads
    plain = np.arange(K3)
    old = [conflicts(plain[e], group) for name, group, e in acc if name.startswith("stage 3")]
    print("\nstage-3 conflicts per read of the unpadded layout:", sorted(set(old)))
    assert len(old) == 25 and all(c > 0 for c in old)


def test_stages_address_the_same_elements_one_to_one(lds):
    acc = stage_accesses()
    for prefix in ("stage 1 write", "stage 2 read", "stage 2 write", "stage 3 read"):
        e = np.concatenate([el for name, _, el in acc if name.startswith(prefix)])
        assert e.size == K3 and np.array_equal(np.sort(e), np.arange(K3)), prefix
        a = lds[e]
        assert np.array_equal(np.sort(a), np.sort(lds)) and len(set(a.tolist())) == K3, prefix
