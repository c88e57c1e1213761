"""Connected components on the GPU (abnn.h abnn_components_*, csrc/components.hip).

Every comparison is Brain.components against components.reference over the
same brain's download_synapses(), all result words equal, with the LINK step's
path switch (abnn_debug_set_components_path) at 0, 1 and 2 wherever the settled
map could apply: record-count edges, chains and a ring, contention (a star, one
pair, a large uniform graph, disjoint pairs, cliques at the bin edges), graphs
without a giant component, percolation on the generated graph, neuron ids up to
the last valid one, tombstones and capacity headroom, a structural update, the
enqueue-only path on a side stream between passes, the step path over shards,
the C++ mirrors and the device allocations."""
import ctypes as C
import json
import socket
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
NONE = 0xFFFFFFFF
INF = float("inf")
# the special weights of tests/test_hops_gpu.py
SPECIAL = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-40, 127.99999, 128.0, -128.0, -127.99999, 0.001, 2.0 ** -24,
                    2.0 ** -25, -(2.0 ** -24)], dtype=F32)
BIG = 3_000_001  # every workgroup loops more than once; the last record is in no 16-byte load
BIG_NRN = 100_512
PATHS = (0, 1, 2)


def _set_path(b, path):
    from abnn_amd import _lib

    _lib.call("abnn_debug_set_components_path", b._h, path)


def _words(d):
    from abnn_amd import components

    return components.to_words(d)


def _same(got, want, what=""):
    g, w = _words(got), _words(want)
    assert g.shape == w.shape, what
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (what, bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist())
    assert got["gave_up"] == 0, what


def _against_reference(b, neurons=None, weights=None, sizes=False, syn=None, paths=PATHS, note="", want=None):
    from abnn_amd import components

    syn = b.download_synapses() if syn is None else syn
    if want is None:
        want = components.reference(syn, components.config(neurons, weights, sizes, b.n_neuron()), b.n_neuron())
    got = None
    for path in paths:
        _set_path(b, path)
        got = b.components(neurons, weights, sizes)
        _same(got, want, f"{note} path {path} neurons {neurons} weights {weights} sizes {sizes}")
    _set_path(b, 0)
    return got


def _syn(src, dst, w=0.5):
    from abnn_amd import SYN_DTYPE

    syn = np.zeros(len(src), dtype=SYN_DTYPE)
    syn["src"], syn["dst"], syn["w"] = src, dst, w
    return syn


def _records(n, seed, n_nrn=1000):
    """Seeded records as tests/test_hops_gpu.py plants them: uniform src / dst,
    weights in [-0.1, 1.1] and the special values at the first, a middle and
    the last index."""
    rng = np.random.default_rng(seed)
    syn = _syn(rng.integers(0, n_nrn, n, dtype=np.uint32), rng.integers(0, n_nrn, n, dtype=np.uint32),
               rng.uniform(-0.1, 1.1, n).astype(F32))
    k = len(SPECIAL)
    if n >= 3 * k:
        for at in (0, n // 2 - k // 2, n - k):
            syn["w"][at:at + k] = SPECIAL
    else:
        for j, at in enumerate(sorted({0, n // 2, n - 1})):
            syn["w"][at] = SPECIAL[(seed + j) % k]
    return syn


def _brain(n_syn, n_hidden=488, **kw):
    import abnn_amd

    return abnn_amd.Brain(256, 256, n_hidden, n_syn, 100_000, **kw)


def _upload(b, syn):
    b.upload_synapses(syn)
    back = b.download_synapses()
    assert np.array_equal(back.view(np.uint32), syn.view(np.uint32))
    return back


# ---- 1. record-count edges ---------------------------------------------------------------------
# 4096 records are one workgroup iteration (2 x 512 threads x 4 loads): 4095 .. 4097 cross it with and without
# the odd last record, 8193 is two iterations and that record.  With the path at 2 the leading slice is half
# of the records (rounded down to even), so every one of these sizes also moves the slice's edge.
@pytest.mark.parametrize("n_syn", [1, 2, 3, 63, 64, 65, 4095, 4096, 4097, 8193])
def test_record_count_edges(gpu, n_syn):
    with _brain(n_syn) as b:
        syn = _records(n_syn, n_syn)
        if n_syn < 300:  # sparse: make some components larger than a pair
            syn["src"][::3] = 300
        back = _upload(b, syn)
        for neurons in (None, (256, 700), (999, 1)):
            for weights in (None, (0.25, 0.9), (-INF, INF)):
                for sizes in (False, True):
                    got = _against_reference(b, neurons, weights, sizes, syn=back, note=f"n {n_syn}")
                    assert got["records"] == n_syn and got["neurons"] == 1000
                    assert ("sizes" in got) == sizes


# ---- 2. chains -----------------------------------------------------------------------------------
CHAIN = 100_000


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_a_path_over_100000_neurons(gpu, order):
    src = np.arange(CHAIN - 1, dtype=np.uint32)
    if order == "descending":
        src = src[::-1].copy()
    elif order == "shuffled":
        src = np.random.default_rng(3).permutation(src)
    syn = _syn(src, src + 1)
    with _brain(len(syn), n_hidden=CHAIN - 512) as b:
        assert b.n_neuron() == CHAIN
        b.upload_synapses(syn)
        got = _against_reference(b, sizes=True, syn=syn, note=order)
        assert (got["components"], got["largest"], got["largest_label"], got["singletons"], got["gave_up"]) == (1, CHAIN, 0, 0, 0)
        assert not got["labels"].any() and (got["sizes"] == CHAIN).all() and got["bins"][16] == 1
        half = _against_reference(b, (CHAIN // 2, CHAIN // 2), syn=syn, note=order)  # the upper half alone
        assert (half["components"], half["largest_label"]) == (1, CHAIN // 2)


def test_a_ring(gpu):
    from abnn_amd import graph

    with _brain(2000) as b:
        b.build_graph(graph.spec([graph.small_world((0, 1000), 2, 0.0, graph.uniform(0.0, 1.0))], 1))
        syn = b.download_synapses()
        got = _against_reference(b, syn=syn)
        assert (got["components"], got["largest"], got["gave_up"]) == (1, 1000, 0)
        cut = _against_reference(b, weights=(0.5, INF), sizes=True, syn=syn)  # about half of the edges: arcs
        assert cut["components"] > 100 and cut["largest"] < 100


# ---- 3. contention -------------------------------------------------------------------------------
def test_a_star_and_one_pair(gpu):
    n = 50_001
    rng = np.random.default_rng(1)
    star = _syn(np.full(n, 7, dtype=np.uint32), rng.integers(0, 1000, n, dtype=np.uint32))
    star["src"][::2], star["dst"][::2] = star["dst"][::2].copy(), 7  # the hub on either side
    pair = _syn(np.full(n, 998, dtype=np.uint32), np.full(n, 3, dtype=np.uint32))
    pair["src"][1::2], pair["dst"][1::2] = 3, 998
    with _brain(n) as b:
        b.upload_synapses(star)
        got = _against_reference(b, syn=star, note="star")
        assert got["components"] == 1 and got["largest"] == 1000
        b.upload_synapses(pair)
        got = _against_reference(b, sizes=True, syn=pair, note="pair")
        assert (got["components"], got["largest"], got["largest_label"], got["singletons"]) == (999, 2, 3, 998)
        assert got["labels"][998] == 3 and got["sizes"][998] == 2 == got["sizes"][3]


@pytest.fixture(scope="module")
def big():
    """One brain of 3 000 001 records over 100 512 neurons, uploaded once, and the
    references of the tests below; they only read it."""
    import abnn_amd
    from abnn_amd import components

    syn = _records(BIG, 5, BIG_NRN)
    syn.setflags(write=False)
    b = abnn_amd.Brain(256, 256, 100_000, BIG, 100_000)
    b.upload_synapses(syn)
    want = {}
    for key, (neurons, weights, sizes) in {"all": (None, None, True), "heavy": (None, (1.096, INF), False)}.items():
        want[key] = components.reference(syn, components.config(neurons, weights, sizes, BIG_NRN), BIG_NRN)
    yield b, syn, want
    b.close()


def test_big_uniform_graph(gpu, big):
    b, syn, want = big
    got = _against_reference(b, sizes=True, syn=syn, want=want["all"])
    assert got["records"] == BIG and got["neurons"] == BIG_NRN
    assert got["components"] == 1 and got["largest"] == BIG_NRN  # 60 records per neuron: one giant component
    # a threshold that leaves about one record per ten neurons (0.004 / 1.2 of them): fragments
    frag = _against_reference(b, weights=(1.096, INF), syn=syn, want=want["heavy"])
    assert frag["components"] > BIG_NRN // 2 and frag["largest"] < 1000


def test_two_runs_give_equal_words(gpu, big):
    b, syn, want = big
    for path in PATHS:
        _set_path(b, path)
        a, c = b.components(sizes=True), b.components(sizes=True)
        assert np.array_equal(_words(a), _words(c))
    _set_path(b, 0)


def test_disjoint_pairs_and_cliques(gpu):
    n_nrn = 1000
    i = np.arange(n_nrn // 2, dtype=np.uint32)
    pairs = _syn(2 * i, 2 * i + 1)
    pairs = np.concatenate([pairs, pairs[::-1], pairs])  # every pair three times, both directions of travel
    with _brain(len(pairs)) as b:
        b.upload_synapses(pairs)
        got = _against_reference(b, sizes=True, syn=pairs, note="pairs")
        assert got["components"] == n_nrn // 2 and got["bins"][1] == n_nrn // 2 and got["bins"].sum() == n_nrn // 2
        assert (got["largest"], got["largest_label"], got["singletons"]) == (2, 0, 0)
        assert np.array_equal(got["labels"], np.arange(n_nrn) // 2 * 2) and (got["sizes"] == 2).all()
    # cliques of sizes 1, 2, 3, 4, 7, 8 at the bin edges, from neuron 100 on, highest id first in every record
    src, dst, at, first = [], [], 100, {}
    for size in (1, 2, 3, 4, 7, 8):
        first[size] = at
        for u in range(at, at + size):
            for v in range(at, u):
                src.append(u)
                dst.append(v)
        at += size
    cl = _syn(np.array(src, dtype=np.uint32), np.array(dst, dtype=np.uint32))
    with _brain(len(cl)) as b:
        b.upload_synapses(cl)
        got = _against_reference(b, (100, 25), sizes=True, syn=cl, note="cliques")
        assert got["components"] == 6 and got["bins"][:4].tolist() == [1, 2, 2, 1] and got["singletons"] == 1
        assert (got["largest"], got["largest_label"]) == (8, first[8])
        for size, f in first.items():
            assert (got["labels"][f:f + size] == f).all() and (got["sizes"][f:f + size] == size).all()
        _against_reference(b, sizes=True, syn=cl, note="cliques, every neuron")


# ---- 4. no giant component -----------------------------------------------------------------------------
def test_all_singletons_and_two_equal_halves(gpu):
    n_nrn = 1000
    loops = _syn(np.arange(n_nrn, dtype=np.uint32), np.arange(n_nrn, dtype=np.uint32))  # self-loops join nothing
    with _brain(n_nrn) as b:
        b.upload_synapses(loops)
        got = _against_reference(b, sizes=True, syn=loops, note="self-loops")
        assert (got["followed"], got["components"], got["singletons"], got["largest"], got["largest_label"]) == (
            n_nrn, n_nrn, n_nrn, 1, 0)
        assert got["bins"][0] == n_nrn and np.array_equal(got["labels"], np.arange(n_nrn))
    with _brain(0) as b:  # no records at all
        for path in PATHS:
            _set_path(b, path)
            got = b.components((10, 5), sizes=True)
            assert (got["records"], got["components"], got["singletons"], got["largest"], got["largest_label"]) == (0, 5, 5, 1, 10)
            assert got["labels"][10:15].tolist() == [10, 11, 12, 13, 14] and int((got["labels"] == NONE).sum()) == 995
            assert got["sizes"][10:15].tolist() == [1] * 5 and not got["sizes"][15:].any()
    # two halves of equal size, interleaved: even ids and odd ids; the majority sample may pick either
    rng = np.random.default_rng(8)
    n = 20_000
    u, v = rng.integers(0, n_nrn // 2, n, dtype=np.uint32), rng.integers(0, n_nrn // 2, n, dtype=np.uint32)
    odd = rng.integers(0, 2, n, dtype=np.uint32)
    halves = _syn(2 * u + odd, 2 * v + odd)
    with _brain(n) as b:
        b.upload_synapses(halves)
        got = _against_reference(b, sizes=True, syn=halves, note="halves")
        assert (got["components"], got["largest"], got["largest_label"]) == (2, n_nrn // 2, 0)
        assert np.array_equal(got["labels"], np.arange(n_nrn) % 2)


# ---- 5. percolation on the generated graph ---------------------------------------------------------------
def test_percolation_on_the_generated_graph(gpu):
    with _brain(1_000_000, n_hidden=99_488) as b:
        b.build_random_graph(1)
        syn = b.download_synapses()
        w = syn["w"][np.isfinite(syn["w"])]
        last = None
        for q in (0.0, 0.5, 0.9, 0.97, 0.995):
            t = float(np.quantile(w, q)) if q else -INF
            got = _against_reference(b, weights=(t, INF), syn=syn, note=f"t {t}")
            assert last is None or (got["components"] >= last["components"] and got["largest"] <= last["largest"])
            last = got
        assert last["components"] > 50_000  # 0.5 % of ten records per neuron: the network has fallen apart
        whole = _against_reference(b, syn=syn)
        assert whole["largest"] > 90_000
        _against_reference(b, (0, 512), sizes=True, syn=syn)  # inputs and outputs: the dense block


# ---- 6. high ids, records that are no edge, tombstones, headroom --------------------------------------------
def _hip():
    with open("/proc/self/maps") as f:  # the HIP runtime the library loaded, not a second one
        loaded = {line.split()[-1] for line in f if "libamdhip64.so" in line}
    assert len(loaded) == 1, loaded
    hip = C.CDLL(loaded.pop())
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


def test_high_neuron_ids(gpu):
    import abnn_amd

    n_nrn = (1 << 24) - 3  # odd: the planes are padded
    last = n_nrn - 1
    edges = []
    for base in (1 << 16, 1 << 18, 1 << 23):
        edges += [(i, i + 1) for i in range(base - 3, base + 3)]
    edges += [(last - 2, last - 1), (last, last - 1), (last, 5), (5, 6), (6, (1 << 23) - 3), ((1 << 16) + 3, (1 << 18) - 3)]
    rng = np.random.default_rng(9)
    n_syn = 3001
    syn = _syn(rng.integers(0, n_nrn, n_syn, dtype=np.uint32), rng.integers(0, n_nrn, n_syn, dtype=np.uint32),
               rng.uniform(0.0, 1.0, n_syn).astype(F32))
    at = rng.choice(n_syn, len(edges) + 4, replace=False)
    at[0] = n_syn - 1  # the record that no whole load holds
    for k, (s, d) in zip(at, edges):
        syn["src"][k], syn["dst"][k] = s, d
    bad = at[len(edges):]
    syn["src"][bad[2:]] = syn["dst"][bad[2:]] = NONE  # two tombstones
    hip = _hip()
    with abnn_amd.Brain(256, 256, n_nrn - 512, n_syn, 100_000) as b:
        assert b.n_neuron() == n_nrn
        b.upload_synapses(syn)
        # records that no upload validates, written into the {dst, w} array as abnn_state_ptrs allows: a dst that is
        # N_NRN, a dst far above it, and a live record on a tombstone's src code (a src that is no neuron)
        base, nbytes, elem = b.synapse_layout()["arrays"]["dst_w"]
        assert elem == 8 and nbytes >= n_syn * 8
        for k, dst in ((bad[0], n_nrn), (bad[1], 0xFFFFFFFE), (bad[2], 7)):
            rec = np.array([dst, np.array([0.5], dtype=F32).view(np.uint32)[0]], dtype=np.uint32)
            assert hip.hipMemcpy(base + int(k) * 8, rec.ctypes.data, 8, 1) == 0  # hipMemcpyHostToDevice
        syn = b.download_synapses()
        assert syn["dst"][bad].tolist() == [n_nrn, 0xFFFFFFFE, 7, NONE] and syn["src"][bad[2]] >= n_nrn
        got = _against_reference(b, sizes=True, syn=syn, paths=(1, 2))
        assert got["labels"][last] == 5 == got["labels"][(1 << 23) + 3] and got["followed"] == n_syn - 4
        assert got["labels"][(1 << 18) + 3] == got["labels"][(1 << 16) - 3]
        sub = _against_reference(b, (last - 2, 3), syn=syn, paths=(0, 2))  # the last three ids alone
        assert sub["labels"][last - 2:].tolist() == [last - 2] * 3 and sub["components"] == 1


def test_tombstones_and_capacity_headroom(gpu):
    syn = _records(5_000, 3)
    rng = np.random.default_rng(4)
    dead = rng.choice(5_000, 500, replace=False)
    syn["src"][dead] = NONE
    syn["dst"][dead] = NONE
    with _brain(5_000, syn_capacity=9_000) as b:
        b.upload_synapses(syn)
        back = b.download_synapses()
        assert int((back["dst"] == NONE).sum()) == 500
        got = _against_reference(b, sizes=True, syn=back)
        assert got["records"] == 5_000 and got["followed"] == 4_500
        _against_reference(b, (256, 256), (0.25, 0.9), syn=back)


def test_after_a_structural_update_that_shrank_n_syn(gpu):
    import abnn_amd

    n_syn = 120_000
    b = abnn_amd.Brain(256, 256, 3000, n_syn, n_syn, syn_capacity=n_syn + 1_000, seed=13,
                       w_prune=0.105, p_new=0.0, w_init=0.5, compact_every=2)  # pruning, no growth
    b.build_random_graph(21)
    syn = b.download_synapses()
    dead = np.random.default_rng(6).choice(np.arange(65_536, n_syn), 20_000, replace=False)  # hidden -> hidden records
    syn["src"][dead] = NONE
    syn["dst"][dead] = NONE
    b.upload_synapses(syn)
    before = _against_reference(b, syn=syn)
    b.set_auto_stimulus(0, 256)
    b.encode_traversal(2)  # the second pass runs the structural update: the tombstones are removed
    assert b.n_syn() <= n_syn - 20_000
    after_syn = b.download_synapses()
    assert len(after_syn) == b.n_syn() and not (after_syn["dst"] == NONE).any()
    after = _against_reference(b, sizes=True, syn=after_syn)
    assert after["records"] == b.n_syn() < before["records"]
    _against_reference(b, (512, 3000), (0.2, INF), syn=after_syn)
    b.close()


# ---- 7. the enqueue-only path ------------------------------------------------------------------------------
def test_enqueue_between_passes_on_a_side_stream(gpu, monkeypatch):
    import torch

    import abnn_amd
    from abnn_amd import components
    from test_gpu_indexed import index_state, mask_dirty

    monkeypatch.setenv("ABNN_INDEXED", "2")  # the indexed pass whenever its index is valid
    monkeypatch.setenv("ABNN_INDEX_AFTER", "1")

    def make():
        b = abnn_amd.Brain(256, 256, 99_488, 1_000_000, 1_000_000)
        b.build_random_graph(1)
        b.set_auto_stimulus(0, 256)
        return b

    a, twin = make(), make()
    n_nrn = a.n_neuron()
    cfgs = [components.config(None, None, True, n_nrn), components.config((512, 99_488), (0.5, INF), False, n_nrn),
            components.config(None, None, True, n_nrn)]  # the first config again: the scratch is reused
    outs = [torch.zeros(components.n_words(c, n_nrn), dtype=torch.int64, device="cuda:0") for c in cfgs]
    a.components((0, 1))  # the handle's first call allocates the scratch: it may synchronise
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=0)
    a.encode_traversal(6, stream=side)  # the weights move from the fourth pass
    side.synchronize()
    before = index_state(a)
    assert before["built"] and before["last_indexed"] and mask_dirty(a) == 0
    for path, (c, o) in zip((0, 2, 1), zip(cfgs, outs)):
        _set_path(a, path)
        a.components_enqueue(c, o.data_ptr(), stream=side)
    after = index_state(a)
    assert {k: after[k] for k in ("built", "entries", "max_degree", "indexed_passes")} == {
        k: before[k] for k in ("built", "entries", "max_degree", "indexed_passes")}  # the src index is kept
    a.encode_traversal(2, stream=side)
    side.synchronize()
    assert index_state(a)["last_indexed"] and mask_dirty(a) == 0  # neither the marks nor the mask were touched
    twin.encode_traversal(6)
    syn = twin.download_synapses()
    got = [components.decode(o.cpu().numpy().view(np.uint64), c, n_nrn) for c, o in zip(cfgs, outs)]
    for c, g in zip(cfgs, got):
        _same(g, components.reference(syn, c, n_nrn))
    assert np.array_equal(_words(got[0]), _words(got[2]))
    twin.encode_traversal(2)
    assert index_state(twin)["indexed_passes"] == index_state(a)["indexed_passes"]
    assert a.checksum() == twin.checksum()  # the search wrote nothing but its result
    assert np.array_equal(a.download_synapses().view(np.uint32), twin.download_synapses().view(np.uint32))
    assert np.array_equal(a.last_fired(), twin.last_fired()) and a.scalars() == twin.scalars()
    assert a.stats() == twin.stats()
    # refused on the host, before any launch
    for bad in (components.config((5, 0)), components.config((n_nrn - 1, 2)), components.config((0, 1), (0.5, 0.5))):
        with pytest.raises(abnn_amd.AbnnError) as err:
            a.components_enqueue(bad, outs[0].data_ptr())
        assert err.value.status == 1
    for step in (4, 5, 0xFFFFFFFF):
        with pytest.raises(abnn_amd.AbnnError) as err:
            a.components_step_enqueue(cfgs[0], step, outs[0].data_ptr())
        assert err.value.status == 1
    for planes, n_planes in ((0, 1), (outs[1].data_ptr(), 0)):
        with pytest.raises(abnn_amd.AbnnError) as err:
            a.components_merge_enqueue(cfgs[0], planes, n_planes, outs[0].data_ptr())
        assert err.value.status == 1
    with pytest.raises(abnn_amd.AbnnError) as err:
        a.components_enqueue(cfgs[0], outs[0].data_ptr() + 4)  # misaligned
    assert err.value.status == 1
    a.close()
    twin.close()


# ---- 8. steps and shards -------------------------------------------------------------------------------------
def _merged_shards(shards, cfg, n_nrn, paths):
    """BEGIN, LINK, FLATTEN on every handle, the planes gathered into one device
    buffer, MERGE of all of them on every handle, FLATTEN, CLOSE: the decoded results."""
    import torch

    from abnn_amd import components

    words, pw = components.n_words(cfg, n_nrn), (n_nrn + 1) // 2
    outs = [torch.zeros(words, dtype=torch.int64, device="cuda:0") for _ in shards]
    for s, o, path in zip(shards, outs, paths):
        _set_path(s, path)
        for step in (components.BEGIN, components.LINK, components.FLATTEN):
            s.components_step_enqueue(cfg, step, o.data_ptr())
    planes = torch.cat([o[components.PLANE_AT:components.PLANE_AT + pw] for o in outs]).contiguous()
    for s, o in zip(shards, outs):
        s.components_merge_enqueue(cfg, planes.data_ptr(), len(shards), o.data_ptr())
        for step in (components.FLATTEN, components.CLOSE):
            s.components_step_enqueue(cfg, step, o.data_ptr())
        _set_path(s, 0)
    torch.cuda.synchronize()
    return [components.decode(o.cpu().numpy().view(np.uint64), cfg, n_nrn) for o in outs]


def test_merged_shards_equal_the_unsharded_result(gpu):
    import abnn_amd
    from abnn_amd import components
    from abnn_amd.shard import global_events, shard_ranges

    n_syn, events = 10_000, 100_000
    with _brain(n_syn, n_hidden=4489) as whole:  # 5001 neurons (odd: a padded plane), two records per neuron
        n_nrn = whole.n_neuron()
        syn = _records(n_syn, 7, n_nrn)
        whole.upload_synapses(syn)
        ge = global_events(n_syn, events, 3)
        shards = []
        for lo, hi in shard_ranges(n_syn, 3):
            s = abnn_amd.Brain(256, 256, 4489, hi - lo, events, syn_offset=lo, global_events=ge)
            s.upload_synapses(syn[lo:hi])
            shards.append(s)
        for args in ((None, None, True), ((700, 3000), (0.3, 0.9), False), (None, (0.5, INF), True)):
            cfg = components.config(*args, n_nrn)
            want = _against_reference(whole, *args, syn=syn)
            followed = 0
            for (lo, hi), got in zip(shard_ranges(n_syn, 3), _merged_shards(shards, cfg, n_nrn, (1, 2, 0))):
                assert got["records"] == hi - lo
                assert got["followed"] == int(components.followed(syn[lo:hi], cfg, n_nrn).sum())
                followed += got["followed"]
                got["records"], got["followed"] = n_syn, want["followed"]
                _same(got, want, str(args))
            assert followed == want["followed"]
            alone = shards[0].components(*args)
            assert alone["components"] > want["components"]  # one shard holds only some of the edges
        for s in shards:
            s.close()


def test_a_chain_split_by_parity(gpu):
    import abnn_amd
    from abnn_amd import components

    n_nrn = 10_000
    src = np.arange(n_nrn - 1, dtype=np.uint32)
    syn = _syn(src, src + 1)
    parts = [syn[0::2], syn[1::2]]  # each alone N / 2 pieces, together one
    shards = []
    for p in parts:
        s = abnn_amd.Brain(256, 256, n_nrn - 512, len(p), 100_000)
        s.upload_synapses(p)
        shards.append(s)
    assert shards[0].components()["components"] == n_nrn // 2
    assert shards[1].components()["components"] == n_nrn // 2 + 1
    cfg = components.config(None, None, True, n_nrn)
    for paths in ((1, 1), (2, 2)):
        for p, got in zip(parts, _merged_shards(shards, cfg, n_nrn, paths)):
            assert (got["records"], got["followed"], got["gave_up"]) == (len(p), len(p), 0)
            assert (got["components"], got["largest"], got["largest_label"], got["singletons"]) == (1, n_nrn, 0, 0)
            assert not got["labels"].any() and (got["sizes"] == n_nrn).all()
    for s in shards:
        s.close()


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_sharded_brain_components_world1(gpu, monkeypatch):
    import torch.distributed as dist

    from abnn_amd.shard import ShardedBrain, TorchComm

    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(_port()))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        sb = ShardedBrain(TorchComm(), 256, 256, 488, 10_000, 100_000, device=0, native=True)
        sb.brain.build_random_graph(1)
        for args in ((None, None, True), ((512, 488), (0.3, 0.9), False), ((0, 512), None, True), (None, (0.6, INF), False)):
            _same(sb.components(*args), _against_reference(sb.brain, *args), str(args))
        sb.native.close()
        sb.brain.close()
    finally:
        dist.destroy_process_group()


# ---- 9. the C++ mirrors ----------------------------------------------------------------------------------------
def test_cpp_components(gpu):
    from abnn_amd.build import build_components_test

    prog = build_components_test()
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    lines = r.stdout.strip().splitlines()
    assert lines, (r.returncode, r.stderr[-2000:])
    res = json.loads(lines[-1])
    assert r.returncode == 0 and res["ok"], (res, r.stderr[-2000:])
    assert res["records"] == 100_000 and res["neurons"] == 10_000
    assert res["whole_largest"] > 9_000 and res["cut_components"] > res["whole_components"] and res["io_largest"] == 512


# ---- 10. device memory ---------------------------------------------------------------------------------------------
def test_live_allocations_return_after_destroy(gpu):
    from abnn_amd import _lib

    live = lambda: int(_lib.load().abnn_debug_live_allocations())  # noqa: E731
    base = live()
    b = _brain(5_000)
    b.upload_synapses(_records(5_000, 2))
    created = live()
    b.components()
    first = live()
    assert first == created + 4  # the counters, the settled map, the sample's words; the synchronous call's result
    for path in PATHS:
        _set_path(b, path)
        b.components(sizes=True)  # a larger result: the buffer grows once, the old one is freed
        b.components((10, 20), (0.1, 0.9))
    assert live() == first
    b.close()
    assert live() == base
