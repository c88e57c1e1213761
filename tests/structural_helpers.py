"""The structural update (abnn.h, plasticity contract) restated in numpy, and the
catalogue of tombstone patterns the CPU and GPU edge tests share.

removal_reference / append_reference are written from abnn.h's paragraph with
masks and fancy indexing; they are independent of oracle/c1_oracle.c, which
the tests compare them with (tests/test_structural_model.py, no GPU).

Every pattern carries a predicate over describe(): the property it is named
for, in the units the device code works in (4096-record blocks, 16-record
thread runs, 1024-entry scan slices).  The tests assert it, so a changed
constant cannot silently stop a case from reaching its path."""
import functools

import numpy as np

from oracle import oracle as O

# The library does not export its constants; these restate
# abnn_amd/csrc/engine.h (kCompactChunk, kScanThreads) and
# abnn_amd/csrc/kernels.hip (kSwapPer).
BLOCK = 4096   # kCompactChunk: records per entry of the tombstone tally
RUN = 16       # kSwapPer: consecutive records one thread of the fill holds
SLICE = 1024   # kScanThreads: tally entries (and grown slots) per scan slice
TOMB = 0xFFFFFFFF
N_HIDDEN = 3000  # as test_gpu_plasticity._pair
GRAPH_SEED = 21


# ---- the contract ---------------------------------------------------------------------------

def is_tomb(syn):
    return syn["src"] == TOMB


def removal_reference(syn):
    """With D tombstones and m = n - D: the tombstones below m, in index
    order, take the live records of [m, n), in index order; the first m
    records are the result (a copy)."""
    dead = is_tomb(syn)
    m = len(syn) - int(dead.sum())
    out = syn[:m].copy()
    holes = np.flatnonzero(dead[:m])
    fill = m + np.flatnonzero(~dead[m:])
    assert len(holes) == len(fill)  # D - (tombstones of the tail) on both sides
    out[holes] = syn[fill]
    return out


def append_reference(records, grown_in_slot_order, capacity):
    """The grown records appended in (pass, slot) order while len < capacity."""
    room = max(0, int(capacity) - len(records))
    return np.concatenate([records, grown_in_slot_order[:room]])


def describe(dead, n=None):
    """What the device code sees of a tombstone mask over n records."""
    dead = np.asarray(dead, dtype=bool)
    n = len(dead) if n is None else int(n)
    assert len(dead) == n
    D = int(dead.sum())
    m = n - D
    mb = m // BLOCK
    nbn = (n + BLOCK - 1) // BLOCK
    at = np.flatnonzero(dead)
    bf = int(at[0] // BLOCK) if D else None
    bl = int(at[-1] // BLOCK) + 1 if D else None   # one past the last block holding a tombstone
    holes = at[at < m]
    fill = m + np.flatnonzero(~dead[m:])
    # which tail blocks feed which hole blocks (the k-th hole takes the k-th live tail record)
    pairs = np.unique(np.stack([holes // BLOCK, fill // BLOCK]), axis=1) if len(holes) else np.zeros((2, 0), int)
    per_hole = np.bincount(pairs[0] - pairs[0].min()) if pairs.shape[1] else np.zeros(1, int)
    per_tail = np.bincount(pairs[1] - pairs[1].min()) if pairs.shape[1] else np.zeros(1, int)
    return {
        "n": n, "D": D, "m": m, "mb": mb,
        "holes": int(len(holes)),                   # tombstones below m
        "tail_tombs": D - int(len(holes)),          # tombstones in [m, n)
        "first_block": bf, "last_block": None if bl is None else bl - 1,
        "hole_blocks": (min(bl, mb + 1) - bf if min(bl, mb + 1) > bf else 0) if D and D < n else 0,
        "tail_blocks": nbn - mb if D else 0,
        "hole_offsets": sorted(set((holes % BLOCK).tolist())) if len(holes) <= 64 else None,
        "fill_offsets": sorted(set((fill % BLOCK).tolist())) if len(fill) <= 64 else None,
        "blocks_with_holes": int(len(np.unique(holes // BLOCK))),
        "max_tail_blocks_per_hole_block": int(per_hole.max()),
        "max_hole_blocks_per_tail_block": int(per_tail.max()),
    }


# ---- records --------------------------------------------------------------------------------

def records(n, n_hidden=N_HIDDEN):
    """build_random_graph(21)'s records at 256 + 256 + n_hidden neurons."""
    return O.gen_synapses(0, n, 256, 256, 512 + n_hidden, seed=GRAPH_SEED, nthreads=8)


def with_tombstones(syn, dead):
    syn = syn.copy()
    syn["src"][dead] = TOMB
    syn["dst"][dead] = TOMB
    return syn


def oracle_removal(syn, n_hidden=N_HIDDEN):
    """The oracle's structural update of the records (no pass work: 0 events,
    an update after every pass), as test_structural_update_removal_contract."""
    n = len(syn)
    ob = O.OracleBrain(256, 256, n_hidden, n, 0, compact_every=1, w_prune=0.1, syn_capacity=n)
    ob.set_synapses(syn)
    ob.pass_serial()
    return ob.syn.copy()


# ---- the catalogue --------------------------------------------------------------------------

def _mask(n, at):
    dead = np.zeros(n, dtype=bool)
    dead[np.asarray(at, dtype=np.int64)] = True
    return dead


def _none(n):
    return np.zeros(n, dtype=bool)


def _first(n):
    return _mask(n, [0])


def _last(n):
    return _mask(n, [n - 1])


def _m_boundary(m, tail):
    """D = n - m tombstones: spread over blocks 0 and 1, the last one at m - 1
    (so m = 8193 has a hole in block m / 4096 itself); with `tail`, 37 of them
    lie in the tail instead, the last record among them."""
    def make(n):
        D = n - m
        T = 37 if tail else 0
        below = (np.arange(D - T) * 8190) // (D - T)   # distinct: 8190 / (D - T) > 1
        below[-1] = m - 1
        up = np.concatenate([m + 5 + 101 * np.arange(T - 1), [n - 1]]) if tail else []
        dead = _mask(n, np.concatenate([below, up]))
        assert int(dead.sum()) == D
        return dead
    return make


def _thread_runs_direct(n):
    return _mask(n, [15, 16, 17, 4095, 4096, 4111])


def _thread_runs_scan(n):
    """The same six holes with m = 4112 (a thread-run edge of block 1): the
    tail [4112, n) is dead but for six live records at run edges of its blocks."""
    dead = _thread_runs_direct(n)
    dead[4112:] = True
    dead[[4112, 4113, 4096 + 31, 4096 + 32, 8191, 8192]] = False
    return dead


def _one_hole_three_tail(n):
    """Block 0: 4000 tombstones; the tail [m, n) = 16000 records, three in four dead."""
    idx = np.arange(n)
    return (idx < 4000) | ((idx >= n - 16000) & (idx % 4 != 0))


def _one_tail_three_hole(n):
    """300 tombstones in each of blocks 0, 1, 2 and five near the end."""
    idx = np.arange(n)
    dead = (idx < 3 * BLOCK) & (idx % BLOCK < 3900) & (idx % BLOCK % 13 == 1)
    dead[[20000, 20100, n - 9, n - 3, n - 1]] = True
    return dead


def _tail_only(n):
    return np.arange(n) >= n - 3000


def _all(n):
    return np.ones(n, dtype=bool)


def _every_other(n):
    return np.arange(n) % 2 == 1


# the four of test_gpu_plasticity.test_structural_update_in_place_patterns,
# scaled to n (part 5 runs passes after them)
def _spread(n):
    idx = np.arange(n)
    return (idx % 7 == 3) | (idx == 0) | (idx == n - 1)


def _dense_block(n):
    idx = np.arange(n)
    return (idx >= n // 12) & (idx < n // 2) | (idx % 97 == 5) & (idx < n - n // 2)


def _almost_all(n):
    return np.arange(n) % 1000 != 17


SIZE_EDGES = (1, 15, 16, 17, 4095, 4096, 4097, 8191, 8192, 8193, 12_289, 12_301)
BIG = 2 * 1025 * BLOCK + 1
MID = 5 * BLOCK + 7

# name -> (n -> dead mask, sizes, describe() -> bool, the path it was built for)
PATTERNS = {
    "none": (_none, SIZE_EDGES, lambda d: d["D"] == 0, "no tombstone: the update is a no-op"),
    "first": (_first, SIZE_EDGES, lambda d: d["D"] == 1 and d["first_block"] == 0 and
              (d["holes"] == 1) == (d["n"] > 1), "record 0 takes record n - 1 (n = 1: nothing stays)"),
    "last": (_last, SIZE_EDGES, lambda d: d["D"] == 1 and d["holes"] == 0 and d["tail_tombs"] == 1,
             "record n - 1: a tail tombstone, nothing below m to fill"),
    "thread_runs_direct": (_thread_runs_direct, (8193,), lambda d: d["tail_tombs"] == 0 and d["holes"] == 6 and
                           d["hole_offsets"] == [0, RUN - 1, RUN, RUN + 1, BLOCK - 1],
                           "holes at a thread's last and first record, direct path"),
    "thread_runs_scan": (_thread_runs_scan, (8193,), lambda d: d["tail_tombs"] > 0 and d["m"] % BLOCK == RUN and
                         d["hole_offsets"] == [0, RUN - 1, RUN, RUN + 1, BLOCK - 1] and
                         d["fill_offsets"] == [0, RUN, RUN + 1, 2 * RUN - 1, 2 * RUN, BLOCK - 1],
                         "holes and the tail's live records at thread-run edges, scan path"),
    "one_hole_three_tail": (_one_hole_three_tail, (MID,), lambda d: d["blocks_with_holes"] == 1 and d["tail_tombs"] > 0 and
                            d["max_tail_blocks_per_hole_block"] >= 3, "one hole block's ranks span >= 3 toff intervals"),
    "one_tail_three_hole": (_one_tail_three_hole, (MID,), lambda d: d["hole_blocks"] >= 3 and d["tail_tombs"] > 0 and
                            d["max_hole_blocks_per_tail_block"] >= 3, "one tail block feeds three hole blocks, scan path"),
    "tail_only": (_tail_only, (10_000,), lambda d: d["holes"] == 0 and d["tail_tombs"] == 3000 and d["m"] == 7000,
                  "all tombstones in the tail: nothing moves"),
    "all": (_all, (1, 10_000), lambda d: d["m"] == 0 and d["D"] == d["n"] and d["hole_blocks"] == 0,
            "every record dies: m = 0"),
    "every_other_big": (_every_other, (BIG,), lambda d: d["hole_blocks"] > SLICE and d["tail_blocks"] > SLICE and
                        d["tail_tombs"] > 0, "second slice of the two-launch scan, second round of the tail scan"),
    "spread": (_spread, (MID, 120_000), lambda d: d["tail_tombs"] > 0 and d["holes"] > 0, "scan path, then passes"),
    "dense_block": (_dense_block, (MID, 120_000), lambda d: d["tail_tombs"] == 0 and d["hole_blocks"] > 1,
                    "direct path, then passes"),
    "almost_all": (_almost_all, (MID, 120_000), lambda d: d["m"] * 500 < d["n"] and d["m"] > 0,
                   "the array shrinks a thousandfold (n_ranges shrinks), then passes"),
}
for _m in (8191, 8192, 8193):
    for _tail in (False, True):
        PATTERNS[f"m{_m}_{'scan' if _tail else 'direct'}"] = (
            _m_boundary(_m, _tail), (12_288, 12_301),
            lambda d, _m=_m, _tail=_tail: d["m"] == _m and (d["tail_tombs"] > 0) == _tail and d["first_block"] == 0 and
            d["holes"] >= 4000 and d["hole_blocks"] == (_m - 1) // BLOCK + 1 + (1 if _tail and _m % BLOCK == 0 else 0),
            f"m = {_m}: " + ("the last hole block is empty, k_swap_mb reads a block wholly in the tail"
                            if _m % BLOCK == 0 else "m one off a block boundary"))

PASS_PATTERNS = ("dense_block", "spread", "almost_all")  # direct, scan, shrinking: part 5


def cases(big=True):
    """(name, n) of every pattern at every size it runs at."""
    out = [(name, n) for name, (_, sizes, _, _) in PATTERNS.items() for n in sizes]
    return [c for c in out if big or c[1] != BIG]


@functools.lru_cache(maxsize=4)
def case(name, n):
    """(records with the pattern's tombstones, the mask, describe) of one case,
    the predicate asserted.  Shared between the tests that use it: read-only."""
    make, sizes, holds, why = PATTERNS[name]
    assert n in sizes
    dead = make(n)
    d = describe(dead, n)
    assert holds(d), (name, n, why, {k: v for k, v in d.items() if not k.endswith("offsets")})
    syn = with_tombstones(records(n), dead)
    syn.setflags(write=False)
    dead.setflags(write=False)
    return syn, dead, d
