"""CPU check of the structural-update catalogue (tests/structural_helpers.py):
the numpy restatement of abnn.h's removal equals the oracle on every pattern
and size the GPU edge tests run (tests/test_gpu_structural_edges.py), every
pattern has the property it is named for, and the restatement would notice
the kernel mistakes the catalogue was built against: each is applied to a
block-wise model of the device's bookkeeping (off[], toff[], the binary
search, the capacity guard) and must change the named case's records.

Which case notices which mistake (the GPU cases are in
tests/test_gpu_structural_edges.py):
  b1 = min(bl, mb) in swap_hole_range -- the holes of block m / 4096 stay
    tombstones: m8193_* (a hole at 8192), first at n = 17, thread_runs_scan;
    shown below on the block-wise model.
  `lower` dropped in k_swap_scan2 -- the ranks of hole blocks 1024 and 1025
    restart at 0, so they take the first slice's records: every_other_big;
    shown below.
  pos <= cap in k_append_grown -- n_syn is computed apart (added = cap -
    live), so no download of [0, n_syn) changes: the extra record lands at
    index cap, in the arrays' padding.  test_growth_capacity_cut reads that
    record through the device layout and requires it unwritten.
  src32 not moved by move_record -- downloads read the two code streams, so
    only a random-mode pass sees the stale mirror (a filled hole still reads
    as a tombstone and never gates): test_passes_after_update[*-1] then differs
    from the oracle in stats()["pre_gated"] and, once spikes start, in weights.
  toff[mid] < k0 in k_swap_fill's search -- changes no record (below): the
    walk starts one tail block lower, whose ranks all lie below k0."""
import numpy as np
import pytest

import structural_helpers as H
from structural_helpers import BLOCK, SLICE


@pytest.mark.parametrize("name,n", H.cases())
def test_removal_reference_equals_oracle(name, n):
    syn, dead, d = H.case(name, n)  # asserts the pattern's property
    want = H.removal_reference(syn)
    assert len(want) == d["m"] and not H.is_tomb(want).any()
    got = H.oracle_removal(syn)
    assert len(got) == len(want)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # nothing but the filled holes moved
    keep = ~dead[:d["m"]]
    assert np.array_equal(want[keep].view(np.uint32), syn[:d["m"]][keep].view(np.uint32))


def test_removal_reference_hand_cases():
    """The hand-made arrays of test_oracle.test_structural_update_removal_contract."""
    for tombs, expect in [([2, 4], [0, 1, 18, 3, 19] + list(range(5, 18))),
                          ([0], [19] + list(range(1, 19))),
                          ([15, 17, 18], list(range(15)) + [19, 16]),
                          ([19], list(range(19))),
                          (list(range(20)), []),
                          ([0, 7, 17, 18], [16] + list(range(1, 7)) + [19] + list(range(8, 16)))]:
        syn = np.zeros(20, dtype=H.O.SYN_DTYPE)
        syn["src"] = 256 + np.arange(20)
        syn["dst"] = np.arange(20)
        syn = H.with_tombstones(syn, tombs)
        assert H.removal_reference(syn)["dst"].tolist() == expect


def test_append_reference():
    rec = H.records(10)
    grown = H.records(25)[10:]
    for cap, want in [(10, 10), (11, 11), (24, 24), (25, 25), (40, 25), (3, 10)]:
        out = H.append_reference(rec, grown, cap)
        assert len(out) == want
        assert np.array_equal(out.view(np.uint32), H.records(25)[:want].view(np.uint32)) or cap == 3
    assert np.array_equal(H.append_reference(rec, grown, 3).view(np.uint32), rec.view(np.uint32))


# ---- the device's bookkeeping, block by block, with its mistakes on request -------------------

def blockwise_removal(syn, mutate=None):
    """launch_structural_update's removal as the kernels compute it: the tally
    per 4096-record block, the hole blocks' rank offsets by a scan in slices of
    1024 blocks (k_swap_scan1/2), the tail blocks' live prefix (k_swap_tail),
    then per hole block either m + rank (the tail all live) or a binary search
    over the tail prefix and a walk over the tail blocks (k_swap_fill).
    `mutate` names one deliberate mistake."""
    dead = H.is_tomb(syn)
    n = len(syn)
    nbn = (n + BLOCK - 1) // BLOCK
    tally = np.add.reduceat(dead.astype(np.int64), np.arange(0, n, BLOCK)) if n else np.zeros(0, np.int64)
    D = int(tally.sum())
    out = syn.copy()
    if D == 0 or D >= n:
        return out[:n - D]
    m = n - D
    mb = m // BLOCK
    nz = np.flatnonzero(tally)
    bf, bl = int(nz[0]), int(nz[-1]) + 1
    b0, b1 = bf, min(bl, mb if mutate == "b1_excludes_mb" else mb + 1)
    b1 = max(b1, b0)
    below_mb = int(dead[mb * BLOCK:m].sum())
    tail_tombs = int(dead[m:].sum())
    off = {}
    for s0 in range(b0, b1, SLICE):  # one scan slice per workgroup
        t = tally[s0:min(s0 + SLICE, b1)]
        lower = 0 if mutate == "no_lower" else int(tally[b0:s0].sum())
        pre = np.concatenate([[0], np.cumsum(t)[:-1]])
        for k, b in enumerate(range(s0, min(s0 + SLICE, b1))):
            off[b] = lower + int(pre[k])
    nt = nbn - mb
    live = [(min(n, (mb + j + 1) * BLOCK) - (m if j == 0 else (mb + j) * BLOCK)) -
            (int(tally[mb + j]) - (below_mb if j == 0 else 0)) for j in range(nt)]
    toff = np.concatenate([[0], np.cumsum(live)]).astype(np.int64)
    for b in range(b0, b1):
        if tally[b] == 0:
            continue
        base, hi = b * BLOCK, min(m, (b + 1) * BLOCK)
        holes = base + np.flatnonzero(dead[base:hi])
        h, k0 = len(holes), off[b]
        if tail_tombs == 0:
            out[holes] = syn[m + k0 + np.arange(h)]
            continue
        lo_j, hi_j = 0, nt
        while hi_j - lo_j > 1:
            mid = (lo_j + hi_j) >> 1
            if (toff[mid] < k0) if mutate == "search_strict" else (toff[mid] <= k0):
                lo_j = mid
            else:
                hi_j = mid
        j = lo_j
        while j < nt and toff[j] < k0 + h:
            tlo = m if j == 0 else (mb + j) * BLOCK
            thi = min(n, (mb + j + 1) * BLOCK)
            src = tlo + np.flatnonzero(~dead[tlo:thi])
            r = toff[j] + np.arange(len(src))
            ok = (r >= k0) & (r < k0 + h)
            out[holes[r[ok] - k0]] = syn[src[ok]]
            j += 1
    return out[:m]


def append_with_guard(records, grown, capacity, mutate=None):
    """k_append_grown's guard, slot by slot: record k lands at len + k if that is below the capacity."""
    pos = len(records) + np.arange(len(grown))
    ok = pos <= capacity if mutate == "pos_le_cap" else pos < capacity
    return np.concatenate([records, grown[ok]])


def _equal(a, b):
    return len(a) == len(b) and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name,n", [c for c in H.cases() if c[1] <= 120_000] + [("every_other_big", H.BIG)])
def test_blockwise_model_equals_reference(name, n):
    syn, _, _ = H.case(name, n)
    assert _equal(blockwise_removal(syn), H.removal_reference(syn))


@pytest.mark.parametrize("mutate,name,n", [
    # the holes of block m / 4096 itself are never filled
    ("b1_excludes_mb", "m8193_direct", 12_288),
    ("b1_excludes_mb", "first", 17),
    ("b1_excludes_mb", "m8193_scan", 12_301),
    ("b1_excludes_mb", "thread_runs_scan", 8193),
    # the second slice's ranks restart at 0: its holes take the first slice's records
    ("no_lower", "every_other_big", H.BIG),
])
def test_mistakes_change_the_named_case(mutate, name, n):
    syn, _, _ = H.case(name, n)
    assert not _equal(blockwise_removal(syn, mutate), H.removal_reference(syn))


@pytest.mark.parametrize("name", ["one_tail_three_hole", "one_hole_three_tail", "thread_runs_scan", "spread"])
def test_a_strict_search_is_not_a_mistake(name):
    """`toff[mid] < k0` in k_swap_fill's binary search changes no record: the
    search then starts the walk one tail block lower where toff[j] == k0, all
    of whose ranks lie below k0 and move nothing.  No test can tell the two."""
    syn, _, _ = H.case(name, H.PATTERNS[name][1][0])
    assert _equal(blockwise_removal(syn, "search_strict"), H.removal_reference(syn))


def test_capacity_guard_mistake_changes_the_cut():
    rec, grown = H.records(100), H.records(140)[100:]
    for cap in (100, 101, 107, 139):  # cap_extra 0, 1, 7 and one short of all
        want = H.append_reference(rec, grown, cap)
        assert _equal(append_with_guard(rec, grown, cap), want)
        assert len(append_with_guard(rec, grown, cap, "pos_le_cap")) == len(want) + 1
