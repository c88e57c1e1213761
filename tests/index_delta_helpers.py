"""The delta mark of the indexed pass restated in numpy (DESIGN.md §5 "Indexed
pass"; no GPU): the invariant between the event mask and the marked set, what
one mark launch does to the mask, and the counters it reports.  Shared by
tests/test_index_delta_model.py (the restatement against itself) and
tests/test_gpu_index_delta.py (the device against it).

Bit e of the mask (word e >> 5, bit e & 31) stands for event e; bit n of a
neuron bitmap for neuron n."""
from __future__ import annotations

import numpy as np


def bits_of(words, n):
    """The first n bits of u32 words as a bool array."""
    b = np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little")
    assert b.size >= n
    return b[:n].astype(bool)


def words_of(bits):
    """A bool array as u32 words (padded with zero bits)."""
    pad = (-len(bits)) % 32
    b = np.concatenate([np.asarray(bits, dtype=np.uint8), np.zeros(pad, dtype=np.uint8)])
    return np.packbits(b, bitorder="little").view("<u4")


def expected_mask_bits(src, events, n_nrn, marked_bits):
    """The invariant: bit e (e < events) is set iff src[e] < n_nrn and src[e]
    is in the marked set.  From the records alone, not from the index."""
    s = np.asarray(src[:events], dtype=np.int64)
    live = s < n_nrn
    out = np.zeros(events, dtype=bool)
    out[live] = marked_bits[s[live]]
    return out


def degrees(src, events, n_nrn):
    """Entries per neuron of the index over records [0, events)."""
    s = np.asarray(src[:events], dtype=np.int64)
    return np.bincount(s[s < n_nrn], minlength=n_nrn)


def delta_counts(old_bits, new_bits, deg):
    """{neurons entered, neurons left, entries set, entries cleared} of the
    launch that moves the marked set from old to new."""
    ent, lev = new_bits & ~old_bits, old_bits & ~new_bits
    return [int(ent.sum()), int(lev.sum()), int(deg[ent].sum()), int(deg[lev].sum())]


def index_of(src, events, n_nrn):
    """row / off as the build groups them (the order inside a list is free)."""
    s = np.asarray(src[:events], dtype=np.int64)
    live = np.flatnonzero(s < n_nrn)
    order = live[np.argsort(s[live], kind="stable")]
    row = np.concatenate([[0], np.cumsum(np.bincount(s[live], minlength=n_nrn))])
    return row, order.astype(np.uint32)


def delta_mark(mask_words, old_bits, new_bits, row, off, rng=None):
    """One mark launch on a copy of the mask: an OR per entry of an entering
    neuron, an AND-NOT per entry of a leaving one, in the order rng shuffles
    them into (atomics on distinct bits of one word commute)."""
    mask = np.array(mask_words, dtype="<u4")
    ops = []
    for n in np.flatnonzero(new_bits ^ old_bits):
        ops += [(int(e), bool(old_bits[n])) for e in off[row[n]:row[n + 1]]]
    if rng is not None:
        rng.shuffle(ops)
    for e, leave in ops:
        if leave:
            mask[e >> 5] &= np.uint32(~(1 << (e & 31)) & 0xFFFFFFFF)
        else:
            mask[e >> 5] |= np.uint32(1 << (e & 31))
    return mask
