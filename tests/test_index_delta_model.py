"""The delta mark's logic in numpy alone (tests/index_delta_helpers.py): old
marked set, new marked set and index give the expected mask, whatever the order
of the per-entry operations, with tombstones, records past the sweep, neurons
without a list and sets and clears that share mask words."""
import numpy as np
import pytest

import index_delta_helpers as D

N_NRN, N_SYN, EVENTS = 700, 5000, 4321  # a partial last mask word; records [EVENTS, N_SYN) are not swept


def _records(seed):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, N_NRN - 50, N_SYN).astype(np.uint32)  # the last 50 neurons have no list
    src[0:256] = np.repeat(np.arange(8, dtype=np.uint32), 32)  # 32 entries to a mask word, as the dense block
    src[300:364:2], src[301:364:2] = 600, 601  # two neurons alternating event by event over two words
    src[rng.choice(N_SYN, 200, replace=False)] = 0xFFFFFFFF  # tombstones
    return rng, src


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_delta_keeps_the_invariant(seed):
    rng, src = _records(seed)
    row, off = D.index_of(src, EVENTS, N_NRN)
    deg = D.degrees(src, EVENTS, N_NRN)
    assert off.size == deg.sum() == np.count_nonzero(src[:EVENTS] < N_NRN) and off.max() < EVENTS
    marked = np.zeros(N_NRN, dtype=bool)
    mask = np.zeros((EVENTS + 31) // 32 + 4, dtype=np.uint32)
    sets = [rng.random(N_NRN) < 0.3, rng.random(N_NRN) < 0.3, np.ones(N_NRN, dtype=bool), np.zeros(N_NRN, dtype=bool)]
    swap = np.zeros(N_NRN, dtype=bool)
    swap[600] = True  # 600 enters ...
    # ... and leaves in the launch in which 601 enters, in the same words; then nothing is left
    sets += [swap, np.arange(N_NRN) == 601, np.zeros(N_NRN, dtype=bool)]
    for new in sets:
        ent, lev, n_set, n_clr = D.delta_counts(marked, new, deg)
        before = D.bits_of(mask, EVENTS)
        mask = D.delta_mark(mask, marked, new, row, off, rng)
        after = D.bits_of(mask, EVENTS)
        assert np.array_equal(after, D.expected_mask_bits(src, EVENTS, N_NRN, new))
        assert not D.bits_of(mask, mask.size * 32)[EVENTS:].any()
        assert (np.count_nonzero(after & ~before), np.count_nonzero(before & ~after)) == (n_set, n_clr)
        assert (ent, lev) == (np.count_nonzero(new & ~marked), np.count_nonzero(marked & ~new))
        marked = new
    assert not mask.any()


def test_a_gap_is_a_larger_difference():
    """Marked sets A -> C in one launch give the mask that A -> B -> C gives."""
    rng, src = _records(9)
    row, off = D.index_of(src, EVENTS, N_NRN)
    a, b, c = (rng.random(N_NRN) < 0.2 for _ in range(3))
    zero = np.zeros((EVENTS + 31) // 32, dtype=np.uint32)
    ma = D.delta_mark(zero, np.zeros(N_NRN, dtype=bool), a, row, off)
    via_b = D.delta_mark(D.delta_mark(ma, a, b, row, off), b, c, row, off)
    assert np.array_equal(D.delta_mark(ma, a, c, row, off), via_b)
    assert np.array_equal(D.words_of(D.expected_mask_bits(src, EVENTS, N_NRN, c)), via_b)
