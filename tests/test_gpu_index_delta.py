"""The delta mark of the indexed pass (DESIGN.md §5 "Indexed pass"): the event
mask persists from pass to pass beside a marked set, k_index_mark moves it by
the difference between the marked set and the pass's exact bitmap, and k_gate's
mask flavour only reads it.  Results stay the CPU oracle's on bits; on top of
that, after every pass:

1. abnn_debug_index_mask_dirty is 0 (the device's own expected mask),
2. the downloaded mask is, in numpy and from the downloaded src alone, bit e set
   iff src[e] < N_NRN and src[e] is in the downloaded marked set, and zero at
   and past E,
3. after an indexed pass the marked set is the pass's exact bitmap, and the
   launch's counters are what numpy counts from the two marked sets and the
   neurons' degrees; after any other pass mask and marked set are unchanged.

ABNN_INDEXED=2 and ABNN_INDEX_AFTER=1 as tests/test_gpu_indexed.py; graphs of
at most 2^21 records."""
import ctypes as C

import numpy as np
import pytest

import index_delta_helpers as D
import knob_helpers as K
import test_gpu_indexed as TI

pytestmark = pytest.mark.gpu

CRAFT = (3000, 1 << 17, 1 << 17)  # the dense block and as many sparse records: 256 iterations of 512 events
W = 5  # window_pre's default


@pytest.fixture
def forced(monkeypatch):
    monkeypatch.setenv("ABNN_INDEXED", "2")
    monkeypatch.setenv("ABNN_INDEX_AFTER", "1")


# ---- the debug interface -----------------------------------------------------------------------
def _p32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def mask_copy(g):
    """(mask words, padding included; marked set bits) of a built index."""
    n = g.n_neuron()
    mask = np.zeros(g.visited_events() // 32 + 16384, dtype=np.uint32)  # room for the last iteration and the padding
    marked = np.zeros((n + 31) // 32 + 2, dtype=np.uint32)
    assert g._lib.abnn_debug_index_mask_copy(g._h, _p32(mask), mask.size, _p32(marked), marked.size) == 0
    assert not D.bits_of(marked, marked.size * 32)[n:].any()
    return mask, D.bits_of(marked, n)


def bitmap(g):
    n = g.n_neuron()
    out = np.zeros((n + 31) // 32 + 2, dtype=np.uint32)
    f = g._lib.abnn_debug_bitmap
    f.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(C.c_int)]
    f.restype = C.c_int
    inc = C.c_int(-1)
    assert f(g._h, _p32(out), out.size, C.byref(inc)) == 0
    return D.bits_of(out, n)


def delta(g):
    out = (C.c_uint64 * 4)()
    assert g._lib.abnn_debug_index_delta(g._h, out) == 0
    return [int(v) for v in out]


class Watch:
    """The three checks after every pass of one handle; keeps the mask and the
    marked set of the pass before.  src: the records' as they are now (set it
    again after a writer of src)."""

    def __init__(self, g):
        self.g, self.n = g, g.n_neuron()
        self.refresh()
        self.mask, self.marked = None, np.zeros(self.n, dtype=bool)
        self.log = []  # per indexed pass: the device's counters, the entering and the leaving neurons
        self.total = []  # ... and the entries of its whole marked set

    def refresh(self):
        self.src = self.g.download_synapses()["src"]
        self.events = self.g.visited_events()
        self.deg = D.degrees(self.src, self.events, self.n)

    def check(self, k, indexed):
        g = self.g
        st = TI.index_state(g)
        assert bool(st["last_indexed"]) == indexed, f"pass {k}: {st}"
        assert TI.mask_dirty(g) == 0, f"pass {k}: the mask is not the marked set's"
        if not st["built"]:
            self.mask, self.marked = None, np.zeros(self.n, dtype=bool)
            return
        mask, marked = mask_copy(g)
        bits = D.bits_of(mask, mask.size * 32)
        want = D.expected_mask_bits(self.src, self.events, self.n, marked)
        assert np.array_equal(bits[:self.events], want), f"pass {k}: {np.count_nonzero(bits[:self.events] != want)} bits"
        assert not bits[self.events:].any(), f"pass {k}: bits past E"
        if indexed:
            assert np.array_equal(marked, bitmap(g)), f"pass {k}: the marked set is not the pass's bitmap"
            cnt = delta(g)  # the device's counters
            assert cnt == D.delta_counts(self.marked, marked, self.deg), f"pass {k}"
            self.log.append((cnt, np.flatnonzero(marked & ~self.marked), np.flatnonzero(self.marked & ~marked)))
            self.total.append(int(self.deg[marked].sum()))
        else:
            assert np.array_equal(marked, self.marked), f"pass {k}: the marked set moved in a pass that was not indexed"
            if self.mask is not None:
                assert np.array_equal(mask, self.mask), f"pass {k}: the mask moved in a pass that was not indexed"
        self.mask, self.marked = mask, marked


def step(g, o, w, k, indexed=True, threaded=True, stats=True):
    g.encode_traversal(1)
    if threaded:
        o.pass_threaded(nthreads=16)
    else:
        o.pass_serial()
    K.same(g, o, f"pass {k}")
    if stats:
        assert g.stats() == o.stats(), f"stats, pass {k}"
    w.check(k, indexed)


def clock(o):
    return int(o.scalars()["clock"])


# ---- turnover ----------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [W, 1])
def test_turnover(gpu, forced, window):
    """The generated graph from lastFired = 0: a full mark in the first indexed
    pass, the mass clear when the start-up stamps age out, then a steady state
    in which every launch sets and clears some lists and far from all.

    At 10 records per neuron the default base_scale lets the hidden activity
    die out, and 256 stimulated inputs spend the budget in the dense block, so
    base_scale is 10 and 8 inputs are stimulated (the oracle then shows neurons
    entering and leaving in every pass once the start-up spikes have aged out,
    from pass 2 window_pre + 2 on).  At window_pre = 1 nothing but the stimulus
    survives the start-up (every neuron is refractory while every neuron is
    recent): 3000 hidden neurons stamped recent before pass 3 start it."""
    g, o = K.pair(K.LARGE, K.graph(K.LARGE), window_pre=window, base_scale=10.0)
    for x in (g, o):
        x.set_auto_stimulus(0, 8)
    w = Watch(g)
    passes = 4 * window + 2 if window > 1 else 12
    first_steady = 2 * window + 2 if window > 1 else 5
    seed = np.random.default_rng(3).choice(np.arange(512, 512 + K.LARGE[0]), 3000, replace=False)
    for k in range(passes):
        if window == 1 and k == 3:
            for x in (g, o):
                x.set_timestamps(seed, clock(o) - 1)
        step(g, o, w, k, indexed=k >= 1)
    assert passes >= 3 * window + 2
    assert w.log[0][0][2] == w.deg.sum() and w.log[0][0][3] == 0  # pass 1: every list, from the all-zero mask
    steady = w.log[first_steady - 1:]  # (log[i] is pass i + 1)
    assert len(steady) >= window + 1
    for (cnt, ent, lev), total in zip(steady, w.total[first_steady - 1:]):
        assert cnt[2] > 0 and cnt[3] > 0 and ent.size > 0 and lev.size > 0, cnt
        assert cnt[2] < total, (cnt, total)  # a delta, not a full mark
    if window == 1:  # every spike enters one pass and leaves the next
        for (_, ent, _), (_, _, lev) in zip(steady, steady[1:]):
            hidden = ent[ent >= 256]
            assert np.isin(hidden, lev).all()


# ---- crafted lists -----------------------------------------------------------------------------
LENGTHS = (1, 128, 129, 1024, 1025, 2049)  # kHeavyLen = 128, kHeavyChunk = 1024: light, its edge, one chunk, two, three
CHOSEN = tuple(512 + 40 * i + 7 for i in range(len(LENGTHS)))
SPARE = 512 + 2900


def crafted(lists):
    """CRAFT's generated graph with the neurons of `lists` {neuron: positions}
    holding exactly those records as src, never a dst (nothing makes them fire:
    they are recent only when a test stamps them)."""
    syn = K.graph(CRAFT)
    ids = np.array(sorted(lists), dtype=np.uint32)
    syn["src"][np.isin(syn["src"], ids)] = SPARE
    syn["dst"][np.isin(syn["dst"], ids)] = SPARE
    for n, pos in lists.items():
        assert np.unique(pos).size == len(pos) and min(pos) >= 65536 and max(pos) < CRAFT[2]
        assert not np.isin(syn["src"][pos], ids).any()  # the lists do not overlap
        syn["src"][pos] = n
    return syn


def far_clock(g, o):
    """The clock far past every stamp: only the stimulus stays recent."""
    for x in (g, o):
        x.set_scalars(clock(o) + 1000, 0.0, 0.0)


def test_list_lengths_enter_and_leave(gpu, forced):
    """Lists of 1, 128, 129, 1024, 1025 and 2049 entries, scattered, the 1024
    contiguous from an odd offset (32 entries to a mask word): stamped recent,
    they enter in one launch and leave in one launch, and the counters are
    their lengths' (with whatever else moved in those launches)."""
    rng = np.random.default_rng(11)
    free = np.setdiff1d(np.arange(65536, CRAFT[2]), np.arange(70_000, 71_024))
    pos = rng.permutation(free)
    lists, at = {}, 0
    for n, length in zip(CHOSEN, LENGTHS):
        if length == 1024:
            lists[n] = np.arange(70_000, 71_024)
        else:
            lists[n] = pos[at:at + length]
            at += length
    g, o = K.pair(CRAFT, crafted(lists))
    far_clock(g, o)
    w = Watch(g)
    assert [int(w.deg[n]) for n in CHOSEN] == list(LENGTHS)
    for k in range(2):
        step(g, o, w, k, indexed=k >= 1, threaded=False)
    for x in (g, o):
        x.set_timestamps(list(CHOSEN), clock(o) - 1)
    for k in range(2, 2 + 1 + W + 1):
        step(g, o, w, k, threaded=False)
    cnt, ent, _ = w.log[1]  # pass 2: the launch behind the stamps
    assert np.isin(CHOSEN, ent).all()
    others = ent[~np.isin(ent, CHOSEN)]  # whatever else entered in that launch
    assert (cnt[0] - others.size, cnt[2] - int(w.deg[others].sum())) == (len(CHOSEN), sum(LENGTHS))
    left = [i for i, (_, _, lev) in enumerate(w.log) if np.isin(CHOSEN, lev).any()]
    assert left == [1 + W], left  # stamped clock - 1: recent for window_pre passes, all gone in one launch
    cnt, _, lev = w.log[left[0]]
    assert np.isin(CHOSEN, lev).all()
    others = lev[~np.isin(lev, CHOSEN)]
    assert (cnt[1] - others.size, cnt[3] - int(w.deg[others].sum())) == (len(CHOSEN), sum(LENGTHS))
    assert not w.marked[list(CHOSEN)].any()


def test_enter_and_leave_in_one_word(gpu, forced):
    """P and Q alternate event by event over 7 mask words, far apart in the
    bitmap; P2 and Q2 share a bitmap word (one wave holds both).  P and P2 are
    stamped first; Q and Q2 are stamped so that they enter in the very launch in
    which P and P2 leave: sets and clears in the same mask words, the same
    wave-instructions."""
    p, q, p2, q2 = 512 + 1000, 512 + 2500, 512 + 64 * 20 + 3, 512 + 64 * 20 + 9
    run = np.arange(80_001, 80_001 + 200)
    run2 = np.arange(90_017, 90_017 + 80)
    lists = {p: run[0::2], q: run[1::2], p2: run2[0::2], q2: run2[1::2]}
    g, o = K.pair(CRAFT, crafted(lists))
    far_clock(g, o)
    w = Watch(g)
    for k in range(2):
        step(g, o, w, k, indexed=k >= 1, threaded=False)
    for x in (g, o):
        x.set_timestamps([p, p2], clock(o) - 1)
    for k in range(2, 2 + W):  # P and P2 are recent in these
        step(g, o, w, k, threaded=False)
        assert w.marked[[p, p2]].all() and not w.marked[[q, q2]].any()
    for x in (g, o):
        x.set_timestamps([q, q2], clock(o) - 1)
    step(g, o, w, 2 + W, threaded=False)
    _, ent, lev = w.log[-1]
    assert np.isin([q, q2], ent).all() and np.isin([p, p2], lev).all()
    assert w.marked[[q, q2]].all() and not w.marked[[p, p2]].any()
    step(g, o, w, 3 + W, threaded=False)


# ---- mass clear, heavy clear -------------------------------------------------------------------
def test_mass_clear_and_heavy_clear(gpu, forced):
    """Everything marked, then the clock jumps: all but the stimulus leaves in
    one launch.  The stimulus moves: the old inputs' heavy lists leave window_pre
    passes later, the new ones' enter at once.  The stimulus goes and the clock
    jumps again: the last heavy lists clear and the mask is all-zero."""
    g, o = K.pair(K.LARGE, K.graph(K.LARGE))
    for x in (g, o):
        x.set_auto_stimulus(0, 8)
    w = Watch(g)
    k = 0
    for _ in range(3):
        step(g, o, w, k, indexed=k >= 1)
        k += 1
    assert w.marked.all()
    far_clock(g, o)
    step(g, o, w, k)
    k += 1
    assert np.array_equal(np.flatnonzero(w.marked), np.arange(8))
    cnt = w.log[-1][0]
    assert cnt[1] == w.n - 8 and cnt[3] == w.deg[8:].sum() and cnt[:1] == [0] and cnt[2] == 0
    assert (w.deg[:16] > 128).all()  # the inputs' lists are heavy ones
    for x in (g, o):
        x.set_auto_stimulus(8, 8)
    step(g, o, w, k)
    k += 1
    assert np.isin(np.arange(8, 16), w.log[-1][1]).all() and w.marked[:16].all()
    for _ in range(W + 1):
        step(g, o, w, k)
        k += 1
    assert not w.marked[:8].any() and w.marked[8:16].all()
    assert any(np.isin(np.arange(8), lev).all() for _, _, lev in w.log[-(W + 1):])
    for x in (g, o):
        x.set_auto_stimulus(0, 0)
    far_clock(g, o)
    step(g, o, w, k)
    assert not w.marked.any() and not w.mask.any()
    assert np.isin(np.arange(8, 16), w.log[-1][2]).all() and w.log[-1][0][2] == 0


# ---- gaps --------------------------------------------------------------------------------------
def test_gaps(gpu, forced):
    """Stream and two-kernel passes between the indexed ones, in runs of 1, 2
    and window_pre + 1 (window_pre = 2): they leave mask and marked set alone,
    and the first indexed pass after a gap moves the mask by the whole
    difference.  (base_scale, the stimulus and the stamped neurons: as
    test_turnover, so that there are lists to set and to clear after the gaps.)"""
    g, o = K.pair(K.LARGE, K.graph(K.LARGE), window_pre=2, base_scale=10.0)
    seed = np.random.default_rng(3).choice(np.arange(512, 512 + K.LARGE[0]), 3000, replace=False)
    for x in (g, o):
        x.set_auto_stimulus(0, 8)
    w = Watch(g)
    # (pass 0 is eligible and streams: the index is built in front of pass 1)
    kinds = ("first", "indexed", "stream", "indexed", "two", "stream", "indexed", "stream", "two", "stream", "indexed",
             "indexed")
    for k, kind in enumerate(kinds):
        if k == 2:
            for x in (g, o):
                x.set_timestamps(seed, clock(o) - 1)
        TI.set_indexed(g, 0 if kind == "stream" else 2)
        TI.set_fused(g, kind != "two")
        step(g, o, w, k, indexed=kind == "indexed")
    assert len(w.log) == kinds.count("indexed")
    # (pass 1 marks everything, pass 3 is the mass clear with nothing left to enter)
    assert all(cnt[2] > 0 and cnt[3] > 0 for cnt, _, _ in w.log[2:])


# ---- rebuild, snapshot -------------------------------------------------------------------------
def test_rebuild_starts_from_zero(gpu, forced):
    """A lesion drops the index with its mask and marked set.  Built again
    (under the default rule, which does not admit passes at this size, so that
    the state behind the build can be seen), both are all-zero; the first
    indexed pass marks in full and the passes after it are exact."""
    g, o = K.pair(K.LARGE, K.graph(K.LARGE))
    w = Watch(g)
    for k in range(3):
        step(g, o, w, k, indexed=k >= 1)
    g.edit("kill", src=(300, 4000))
    o.set_synapses(g.download_synapses())
    w.refresh()
    assert not TI.index_state(g)["built"] and TI.mask_dirty(g) == 0
    TI.set_indexed(g, 1)
    for k in range(3, 5):
        step(g, o, w, k, indexed=False)
    assert TI.index_state(g)["built"]
    mask, marked = mask_copy(g)
    assert not mask.any() and not marked.any()
    TI.set_indexed(g, 2)
    for k in range(5, 8):
        step(g, o, w, k)
    # pass 5 (every stamp still recent): every list of the new index, nothing to clear; pass 6: the mass clear
    assert w.log[-3][0][2:] == [int(w.deg.sum()), 0] and w.log[-2][0][3] > 0


def test_neuron_state_rolled_back(gpu, forced):
    """A snapshot's neuron state restored three passes later, the records as
    they are: the index stays, the mask and the marked set are those of the last
    indexed pass, and the next indexed pass moves them to the restored state's
    bitmap.  (base_scale and the stimulus: as test_turnover.)"""
    g, o = K.pair(K.LARGE, K.graph(K.LARGE), base_scale=10.0)
    for x in (g, o):
        x.set_auto_stimulus(0, 8)
    w = Watch(g)
    for k in range(7):
        step(g, o, w, k, indexed=k >= 1)
    snap = g.snapshot()
    saved = (o.last_fired.copy(), o.last_visited.copy(), o.scalars())
    for k in range(7, 10):
        step(g, o, w, k)
    snap.restore("state")
    snap.close()
    o.last_fired[:], o.last_visited[:] = saved[0], saved[1]
    o.set_scalars(saved[2]["clock"], saved[2]["reward"], saved[2]["rbar"], saved[2]["pass_index"])
    assert TI.index_state(g)["built"] and TI.mask_dirty(g) == 0
    mask, marked = mask_copy(g)
    assert np.array_equal(mask, w.mask) and np.array_equal(marked, w.marked)
    for k in range(10, 14):
        step(g, o, w, k)
    cnt = w.log[9][0]  # pass 10: from the bitmap of pass 9 to the one three passes back
    assert cnt[3] > 0, cnt  # what entered in passes 8 and 9 leaves again
