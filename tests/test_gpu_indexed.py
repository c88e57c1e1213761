"""The indexed fused pass (DESIGN.md §5 "Indexed pass"): a src index over the
swept records, a per-pass event mask set by k_index_mark from the exact
recent-spike bitmap, and the mask flavour of k_gate that streams the mask where
the stream flavour streams the 3-B src codes.  Which flavour runs is a matter
of time only, so every result stays what the CPU oracle computes, on bits, pass
by pass: records, lastFired, scalars, rBar's bits, statistics.  The tests force
the flavour with ABNN_INDEXED=2 and ABNN_INDEX_AFTER=1 (the graphs are too
small for the default rule), check through abnn_debug_index_state that the
passes they mean to test were indexed, and through abnn_debug_index_mask_dirty
that the pass left the mask all-zero.  2^21-record graphs with config 2's
neuron counts, as tests/test_gpu_stream_pin.py; the oracle's runs are shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import knob_helpers as K

pytestmark = pytest.mark.gpu

N_SYN = 1 << 21
N_HIDDEN = 99_488
FULL = (N_HIDDEN, N_SYN, N_SYN)  # 4096 iterations of 512 events
ODD = (N_HIDDEN, N_SYN, 1_000_192)  # 1953.5 iterations; records [E, n_syn) live but not swept
TINY = (N_HIDDEN, N_SYN, 200)  # 256 visited events: a sweep shorter than one iteration
SMALL = (3000, 1 << 16, 1 << 16)  # the index itself, against numpy


# ---- the debug interface -----------------------------------------------------------------------
def index_state(g):
    out = (C.c_uint64 * 8)()
    ms = C.c_double(-1.0)
    assert g._lib.abnn_debug_index_state(g._h, out, C.byref(ms)) == 0
    keys = ("built", "entries", "max_degree", "last_indexed", "indexed_passes", "eligible", "mode", "events")
    return dict(zip(keys, (int(v) for v in out)), build_ms=ms.value)


def mask_dirty(g):
    w = C.c_uint64(99)
    assert g._lib.abnn_debug_index_mask_dirty(g._h, C.byref(w)) == 0
    return int(w.value)


def set_indexed(g, mode):
    assert g._lib.abnn_debug_set_indexed(g._h, int(mode)) == 0


def set_fused(g, on):
    assert g._lib.abnn_debug_set_fused(g._h, int(on)) == 0


def index_copy(g):
    st = index_state(g)
    row = np.zeros(g.n_neuron() + 1, dtype=np.uint32)
    off = np.zeros(max(1, st["entries"]), dtype=np.uint32)
    assert g._lib.abnn_debug_index_copy(g._h, row.ctypes.data_as(C.POINTER(C.c_uint32)), row.size,
                                        off.ctypes.data_as(C.POINTER(C.c_uint32)), st["entries"]) == 0
    return row, off[:st["entries"]]


def incremental_next(g):
    """Whether the next pass's bitmap was built in-pass (build_next_ok held)."""
    f = g._lib.abnn_debug_bitmap
    f.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(C.c_int)]
    f.restype = C.c_int
    inc = C.c_int(-1)
    buf = (C.c_uint32 * 1)()
    assert f(g._h, buf, 0, C.byref(inc)) == 0
    return bool(inc.value)


@pytest.fixture
def forced(monkeypatch):
    monkeypatch.setenv("ABNN_INDEXED", "2")
    monkeypatch.setenv("ABNN_INDEX_AFTER", "1")


def assert_indexed_clean(g, k, want=True):
    st = index_state(g)
    assert bool(st["last_indexed"]) == want, f"pass {k}: indexed {st}"
    assert mask_dirty(g) == 0, f"pass {k}: the mask is not clean"
    return st


# ---- shared oracle runs ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_run(shape, passes, params):
    _, o = K.pair(shape, K.graph(shape), gpu=False, **dict(params))
    per_pass = []
    for k in range(passes):
        K.set_rewards(k, K.REWARDS, o)
        o.pass_threaded(nthreads=16)
        per_pass.append((o.last_fired.copy(), o.scalars(), o.stats()))
    return per_pass, o.syn[:int(o.s.dims.n_syn)].copy()


def run_against_oracle(shape, passes, first_indexed=1, **params):
    """`passes` passes of the generated graph, the first first_indexed of them
    streamed (ABNN_INDEX_AFTER) and the rest indexed; everything compared pass
    by pass."""
    per_pass, syn = oracle_run(shape, passes, tuple(sorted(params.items())))
    g, _ = K.pair(shape, K.graph(shape), **params)
    for k in range(passes):
        K.set_rewards(k, K.REWARDS, g)
        g.encode_traversal(1)
        lf, sc, st = per_pass[k]
        assert np.array_equal(g.last_fired(), lf), f"lastFired, pass {k}"
        sg = g.scalars()
        assert (sg["clock"], sg["pass_index"]) == (sc["clock"], sc["pass_index"]), f"pass {k}: {sg} != {sc}"
        assert K.f32_bits(sg["rbar"]) == K.f32_bits(sc["rbar"]), f"rbar, pass {k}"
        assert g.stats() == st, f"stats, pass {k}"
        assert_indexed_clean(g, k, k >= first_indexed)
    got = g.download_synapses()
    assert np.array_equal(got.view(np.uint32), syn.view(np.uint32)), "records"
    return g


def run_pair(g, o, passes, each=None, threaded=True, want=None, stats=True):
    """g and o stepped together and compared after every pass (K.same)."""
    for k in range(passes):
        if each:
            each(k)
        g.encode_traversal(1)
        if threaded:
            o.pass_threaded(nthreads=16)
        else:
            o.pass_serial()
        K.same(g, o, f"pass {k}")
        if stats:
            assert g.stats() == o.stats(), f"stats, pass {k}"
        if want is not None:
            assert_indexed_clean(g, k, want(k))


# ---- parity ------------------------------------------------------------------------------------
def test_startup_and_steady_state(gpu, forced):
    """10 passes from lastFired = 0: in the first window_pre passes every
    neuron is recent, so the mask is all ones and every block takes the
    quarter path with a flush per quarter; then the sparse steady state."""
    g = run_against_oracle(FULL, 10)
    st = index_state(g)
    assert st["built"] and st["indexed_passes"] == 9 and st["events"] == FULL[2]
    assert st["entries"] == FULL[2] and st["max_degree"] >= 256 and st["build_ms"] > 0.0


def test_partial_last_iteration_and_records_past_the_sweep(gpu, forced):
    """1,000,192 of 2^21 records are swept: a partial last iteration, ranges of
    one iteration and of none, neurons whose lists straddle E (their records at
    and past E are not in the index) and recent neurons with no record below E."""
    g = run_against_oracle(ODD, 8)
    assert g.visited_events() == ODD[2]
    st = index_state(g)
    src = g.download_synapses()["src"]
    assert st["entries"] == ODD[2] and st["entries"] < np.count_nonzero(src < g.n_neuron())
    row, off = index_copy(g)
    assert off.max() < ODD[2]
    assert np.count_nonzero(np.diff(row.astype(np.int64)) == 0) > 0  # neurons with no swept record


def test_sweep_shorter_than_one_iteration(gpu, forced):
    g = run_against_oracle(TINY, 6)
    assert g.visited_events() == 256 and index_state(g)["entries"] == 256


@pytest.mark.parametrize("budget", [1, 2560, K.HUGE_BUDGET])
def test_budgets(gpu, forced, budget):
    """The cut inside the first range (1), the default, and no cut at all:
    every pre-gated event goes through the refractory stage past the cut too
    (pre_gated and post_gated are results)."""
    run_against_oracle(FULL, 8, max_spikes=budget)


def test_tombstones_inside_the_sweep(gpu, forced):
    """Hand-placed tombstones {src = dst = 0xFFFFFFFF} in the dense block, the
    sparse part and the last iteration: their src is in no list, so they are
    never marked; the other records of the same neurons still are."""
    syn = K.graph(ODD)
    rng = np.random.default_rng(5)
    at = np.concatenate([np.arange(0, 65536, 7), rng.choice(np.arange(65536, ODD[2]), 5000, replace=False),
                         np.arange(ODD[2] - 300, ODD[2])])
    syn["src"][at] = 0xFFFFFFFF
    syn["dst"][at] = 0xFFFFFFFF
    g, o = K.pair(ODD, syn)
    run_pair(g, o, 8, want=lambda k: k >= 1)
    assert index_state(g)["entries"] == ODD[2] - np.unique(at).size


def test_dense_block_alone_recent(gpu, forced):
    """The clock far past every stamp: only the stimulated inputs are recent,
    so the mask holds the dense input->output block (65,536 consecutive events,
    every one pre-gated: the stage overflows, block after block) and nothing
    else in the first pass.  The host write makes k_bitmap build the bitmaps."""
    g, o = K.pair(FULL, K.graph(FULL))
    for x in (g, o):
        x.set_scalars(1000, 0.0, 0.0)
    run_pair(g, o, 6, want=lambda k: k >= 1)
    assert g.stats()["pre_gated"] >= 6 * 65536


def test_neuron_ids_above_2_18(gpu, forced):
    """The index groups by code_src: ids whose filter code folds and rotates
    (every class n >> 18) decode to their own lists."""
    import high_id_helpers as H

    n_hidden = (1 << 20) + 77_000
    syn = H.high_id_graph(512 + n_hidden)
    shape = (n_hidden, len(syn), len(syn))
    g, o = K.pair(shape, syn)
    run_pair(g, o, 7, want=lambda k: k >= 1)
    row, off = index_copy(g)
    src = syn["src"]
    n = int(src.max())
    assert n >> 18 >= 4
    assert sorted(off[row[n]:row[n + 1]]) == sorted(np.flatnonzero(src == n))


@pytest.mark.parametrize("case", ["clock_inc=2", "window_pre=1", "window_pre=7", "window_pre=9", "clock_inc=2,renorm_thresh=9"])
def test_knobs_off_the_defaults(gpu, forced, case):
    """clock_inc != 1, window_pre at and past the spike-list ring, and a
    renormalisation every few passes: the bitmap comes from the lists or from
    k_bitmap, and k_index_mark reads whichever the pass settled."""
    knobs, rewards = K.KNOBS[case]
    g, o = K.pair(K.LARGE, K.graph(K.LARGE), **knobs)
    run_pair(g, o, 10, each=lambda k: K.set_rewards(k, rewards, g, o), want=lambda k: k >= 1)


def test_default_rule_and_host_writes(gpu, monkeypatch):
    """ABNN_INDEXED=1 with a budget and a stimulus small enough for the rule at
    this size.  A pass is indexed iff the index is built, its bitmap was built
    in-pass by the pass before (build_next_ok held) and window_pre x (max_spikes
    + stimulus) x largest degree <= E / 8.  The start-up passes stream; a host
    write to lastFired, a stamp ahead of the clock and a renormalisation send
    the following passes back to the stream until the lists are exact again."""
    monkeypatch.setenv("ABNN_INDEX_AFTER", "1")
    shape, budget, stim = K.LARGE, 8, 8
    g, o = K.pair(shape, K.graph(shape), max_spikes=budget, renorm_thresh=27)
    for x in (g, o):
        x.set_auto_stimulus(0, stim)
    assert index_state(g)["mode"] == 1
    d = []
    for k in range(36):
        if k == 9:
            for x in (g, o):
                x.set_timestamps([700, 70_000], int(o.scalars()["clock"]) - 1)
        if k == 16:
            for x in (g, o):
                x.set_timestamps([800], int(o.scalars()["clock"]) + 3)  # ahead of the clock
        prebuilt = incremental_next(g)  # (a host write drops what the pass before built)
        g.encode_traversal(1)
        o.pass_threaded(nthreads=16)
        K.same(g, o, f"pass {k}")
        assert g.stats() == o.stats(), f"stats, pass {k}"
        st = index_state(g)
        assert mask_dirty(g) == 0
        rule = st["built"] and prebuilt and 5 * (budget + stim) * st["max_degree"] <= shape[2] // 8
        if k >= 1:  # (pass 0: nothing built yet)
            assert bool(st["last_indexed"]) == bool(rule), f"pass {k}: {st}, prebuilt {prebuilt}"
        d.append(bool(st["last_indexed"]))
    assert g.renormalisations() == 1
    assert not any(d[:5]) and d[8], d  # start-up: every neuron recent, k_bitmap builds the bitmaps
    assert not d[9] and any(d[10:16]), d  # the host write, then the lists again
    assert not d[16] and any(d[17:28]), d  # the stamp ahead of the clock
    assert not d[29] and d[-1], d  # the renormalisation (pass 28 starts above the threshold)


def test_flavours_interleaved(gpu, forced):
    """Indexed, stream (the handle's ABNN_INDEXED toggled), two-kernel (its
    ABNN_FUSED toggled: k_gate + k_apply) and world-1 shard passes in turn on
    one handle: the bitmap buffers, the partition and the spike lists hand
    over between them, in both directions."""
    import torch
    from shard_helpers import GpuShards

    g, o = K.pair(K.LARGE, K.graph(K.LARGE, seed=6))
    gs = GpuShards([g])
    kinds = []
    for k in range(16):
        # (pass 0 is eligible and streams: the index is built in front of pass 1)
        kind = ("indexed", "indexed", "stream", "shard", "indexed", "two", "indexed", "two")[k % 8]
        kinds.append(kind)
        set_indexed(g, 0 if kind == "stream" else 2)
        set_fused(g, kind != "two")
        if kind == "shard":
            gs.pass_()
        else:
            g.encode_traversal(1)
        torch.cuda.synchronize()
        o.pass_threaded(nthreads=16)
        K.same(g, o, f"pass {k} ({kind})")
        assert_indexed_clean(g, k, kind == "indexed" and k >= 1)
    assert g.stats() == o.stats()
    assert index_state(g)["indexed_passes"] == kinds.count("indexed") - 1
    for a, b in (("two", "indexed"), ("indexed", "two"), ("shard", "indexed"), ("stream", "shard")):
        assert (a, b) in set(zip(kinds, kinds[1:])), (a, b)  # the hand-overs this run means to cover


# ---- invalidation ------------------------------------------------------------------------------
def _mutations():
    def upload(g, o):
        part = K.graph(K.LARGE, seed=21)[:5000]
        g.upload_synapses(part, first=1000)
        o.set_synapses(g.download_synapses())

    def kill(g, o):
        g.edit("kill", src=(300, 4000))
        o.set_synapses(g.download_synapses())

    def reorder(g, o):
        g.reorder("random", seed=3)
        o.set_synapses(g.download_synapses())

    return dict(upload=upload, kill=kill, reorder=reorder)


@pytest.mark.parametrize("what", ["upload", "kill", "reorder", "rollback"])
def test_invalidation(gpu, forced, what):
    """After a writer of src the index reports not built, the next pass
    streams, the index is built again (ABNN_INDEX_AFTER passes later) and the
    passes are indexed again; exact throughout."""
    g, o = K.pair(K.LARGE, K.graph(K.LARGE))
    run_pair(g, o, 3, want=lambda k: k >= 1)
    assert index_state(g)["built"]
    if what == "rollback":
        snap = g.snapshot()
        g.edit("kill", src=(300, 4000))  # the records change (and the index goes) ...
        assert not index_state(g)["built"]
        g.encode_traversal(1)
        g.encode_traversal(1)
        assert index_state(g)["built"]
        snap.restore()  # ... and come back, with the state of three passes in
        snap.close()
    else:
        _mutations()[what](g, o)
    st = index_state(g)
    assert not st["built"] and st["entries"] == 0
    run_pair(g, o, 3, want=lambda k: k >= 1, stats=what != "rollback")  # (a roll-back keeps the handle's counters)
    st = index_state(g)
    assert st["built"]
    src = g.download_synapses()["src"]
    assert st["entries"] == np.count_nonzero(src < g.n_neuron())


def test_invalidation_by_the_structural_update(gpu, forced):
    """compact_every = 4 without pruning or synaptogenesis: the handle is
    eligible.  An update that finds no tombstone moves nothing and keeps the
    index.  After a lesion the next update closes the records up: n_syn and E
    shrink, the index (rebuilt since the lesion) is dropped again, the passes
    stay exact, and the index is built again over the records as they now lie."""
    g, o = K.pair(K.LARGE, K.graph(K.LARGE), compact_every=4)
    run_pair(g, o, 4, want=lambda k: k >= 1)  # passes 0..3, then the first update: nothing to do
    assert g.structural_updates() == 1 and index_state(g)["built"]
    g.edit("kill", src=(300, 4000))
    o.set_synapses(g.download_synapses())
    assert not index_state(g)["built"]
    n0 = g.n_syn()
    run_pair(g, o, 3, want=lambda k: k >= 1)  # passes 4..6: rebuilt in front of pass 5
    st = index_state(g)
    assert st["built"] and g.structural_updates() == 1 and st["events"] == n0
    run_pair(g, o, 1, want=lambda k: True)  # pass 7, then the update that moves records
    st = index_state(g)
    assert g.structural_updates() == 2 and g.n_syn() < n0 == K.LARGE[1]
    assert not st["built"] and st["entries"] == 0 and st["events"] == g.visited_events() == g.n_syn()
    run_pair(g, o, 3, want=lambda k: k >= 1)  # passes 8..10
    st = index_state(g)
    src = g.download_synapses()["src"]
    assert st["built"] and st["entries"] == np.count_nonzero(src[:st["events"]] < g.n_neuron()) == g.n_syn()


def test_never_indexed_with_plasticity(gpu, forced):
    """Pruning and synaptogenesis with a structural update every 2 passes: the
    handle is not eligible, no index is ever built, every pass streams."""
    g, o = K.pair(K.LARGE, K.graph(K.LARGE), **K.SP)
    run_pair(g, o, 6, want=lambda k: False)
    st = index_state(g)
    assert g.structural_updates() >= 2 and not st["built"] and st["indexed_passes"] == 0


def test_record_arrays_handed_out(gpu, forced):
    g, o = K.pair(K.WIDE, K.graph(K.WIDE))
    run_pair(g, o, 2, threaded=False, want=lambda k: k >= 1)
    g.synapse_layout()
    st = index_state(g)
    assert not st["built"] and st["entries"] == 0  # its memory went with the hand-out
    run_pair(g, o, 2, threaded=False, want=lambda k: False)
    assert not index_state(g)["built"]


# ---- the index itself --------------------------------------------------------------------------
def test_index_against_numpy(gpu, forced):
    """row / off of a 2^16-record graph with tombstones against numpy's
    grouping of the downloaded src, as sets per neuron."""
    syn = K.graph(SMALL)
    syn["src"][5::97] = 0xFFFFFFFF
    syn["dst"][5::97] = 0xFFFFFFFF
    g, _ = K.pair(SMALL, syn)
    g.encode_traversal(2)
    st = index_state(g)
    assert st["built"] and st["last_indexed"]
    row, off = index_copy(g)
    src = g.download_synapses()["src"].astype(np.int64)
    live = np.flatnonzero(src < g.n_neuron())
    counts = np.bincount(src[live], minlength=g.n_neuron())
    assert row[0] == 0 and np.array_equal(np.diff(row.astype(np.int64)), counts)
    assert st["entries"] == live.size == row[-1] and st["max_degree"] == counts.max()
    order = np.lexsort((off, np.repeat(np.arange(g.n_neuron()), counts)))  # each list sorted
    assert np.array_equal(off[order], live[np.argsort(src[live], kind="stable")])
