"""Reachability on the GPU (abnn.h abnn_hops_*, csrc/hops.hip).

Every comparison is Brain.hops against hops.reference over the same brain's
download_synapses(), all result words equal: record-count edges and the
records that no whole 16-byte load holds, deep searches (a ring, a shuffled
chain), a large uniform graph (many iterations per workgroup, contention on
the plane), the generated graph, neuron ids up to the last valid one,
tombstones and capacity headroom, the enqueue-only path on a side stream,
the step path over shards, and the C++ mirrors."""
import json
import socket
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
NONE = 0xFFFFFFFF
INF = float("inf")
# the special weights of tests/test_degree_gpu.py
SPECIAL = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-40, 127.99999, 128.0, -128.0, -127.99999, 0.001, 2.0 ** -24,
                    2.0 ** -25, -(2.0 ** -24)], dtype=F32)
BIG = 3_000_001  # every workgroup loops more than once; the last record is in no 16-byte load
BIG_NRN = 100_512


def _words(d):
    from abnn_amd import hops

    return hops.to_words(d)


def _same(got, want, what=""):
    g, w = _words(got), _words(want)
    assert g.shape == w.shape, what
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (what, bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist())
    assert got["reached"] == int((got["dist"] != NONE).sum()) == int(got["levels"].sum()), what


def _against_reference(b, seeds, max_hops=64, reverse=False, weights=None, syn=None, note=""):
    from abnn_amd import hops

    syn = b.download_synapses() if syn is None else syn
    got = b.hops(seeds, max_hops, reverse, weights)
    want = hops.reference(syn, hops.config(seeds, max_hops, reverse, weights), b.n_neuron())
    _same(got, want, f"{note} seeds {seeds} H {max_hops} reverse {reverse} weights {weights}")
    return got


def _records(n, seed, n_nrn=1000):
    """Seeded records with uniform src / dst, weights in [-0.1, 1.1] and the
    special values planted at the first, a middle and the last index (all of
    them at each where they fit, else one each, rotated by the seed)."""
    from abnn_amd import SYN_DTYPE

    rng = np.random.default_rng(seed)
    syn = np.zeros(n, dtype=SYN_DTYPE)
    syn["src"] = rng.integers(0, n_nrn, n, dtype=np.uint32)
    syn["dst"] = rng.integers(0, n_nrn, n, dtype=np.uint32)
    syn["w"] = rng.uniform(-0.1, 1.1, n).astype(F32)
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


# ---- 1. record-count edges ---------------------------------------------------------------------
# 4096 records are one workgroup iteration (2 x 512 threads x 4 loads): 4095 .. 4097 cross it with and without
# the odd last record, 8193 is two iterations and that record
@pytest.mark.parametrize("n_syn", [1, 63, 64, 65, 255, 257, 2047, 2049, 10_000, 2, 3, 4095, 4096, 4097, 8193])
def test_record_count_edges(gpu, n_syn):
    with _brain(n_syn) as b:
        for seed in range(3 if n_syn < 3 * len(SPECIAL) else 1):
            syn = _records(n_syn, seed)
            if n_syn < 300:  # sparse: make the seeds' neighbourhoods non-empty
                syn["src"][::3] = [0, 999, 300][seed % 3]
                syn["dst"][1::3] = [999, 0, 511][seed % 3]
            b.upload_synapses(syn)
            back = b.download_synapses()
            assert np.array_equal(back.view(np.uint32), syn.view(np.uint32))
            for seeds in ((0, 1), (999, 1), (256, 256)):
                for reverse in (False, True):
                    for weights in (None, (0.25, 0.9), (-INF, INF)):
                        got = _against_reference(b, seeds, 64, reverse, weights, syn=back, note=f"n {n_syn} seed {seed}")
                        assert got["records"] == n_syn and got["neurons"] == 1000
                        assert got["levels"][0] == seeds[1]


# ---- 2. depth ----------------------------------------------------------------------------------------
def test_a_ring_is_500_hops_deep(gpu):
    from abnn_amd import graph

    with _brain(2000) as b:
        b.build_graph(graph.spec([graph.small_world((0, 1000), 2, 0.0, graph.uniform(0.0, 1.0))], 1))
        syn = b.download_synapses()
        got = _against_reference(b, (0, 1), 1024, syn=syn)
        assert (got["depth"], int(got["levels"][1]), int(got["levels"][500]), got["complete"]) == (500, 2, 1, 1)
        assert got["reached"] == 1000 and not got["levels"][501:].any()
        cut = _against_reference(b, (0, 1), 64, syn=syn)
        assert (int(cut["levels"][64]), cut["reached"], cut["complete"], cut["depth"]) == (2, 129, 0, 64)
        _against_reference(b, (0, 1), 1024, reverse=True, syn=syn)
        _against_reference(b, (0, 1), 1, syn=syn)
    with _brain(4000) as b:
        b.build_graph(graph.spec([graph.small_world((0, 1000), 4, 0.1, graph.uniform(0.0, 1.0))], 1))
        got = _against_reference(b, (0, 1), 64)
        assert (got["depth"], got["reached"], got["complete"]) == (13, 1000, 1)
        _against_reference(b, (0, 1), 64, reverse=True)
        _against_reference(b, (0, 1), 64, weights=(0.5, 1.0))


def test_a_chain_uploaded_in_shuffled_order(gpu):
    from abnn_amd import SYN_DTYPE

    n = 999  # 0 -> 1 -> ... -> 999: the record order says nothing about the hop order
    syn = np.zeros(n, dtype=SYN_DTYPE)
    syn["src"] = np.arange(n)
    syn["dst"] = np.arange(n) + 1
    syn["w"] = 0.5
    syn = syn[np.random.default_rng(3).permutation(n)]
    with _brain(n) as b:
        b.upload_synapses(syn)
        got = _against_reference(b, (0, 1), 1024, syn=syn)
        assert got["depth"] == 999 and got["reached"] == 1000 and (got["levels"][:1000] == 1).all()
        assert np.array_equal(got["dist"], np.arange(1000, dtype=np.uint32))
        back = _against_reference(b, (999, 1), 1024, reverse=True, syn=syn)
        assert np.array_equal(back["dist"], np.arange(1000, dtype=np.uint32)[::-1])
        assert _against_reference(b, (500, 1), 100, syn=syn)["reached"] == 101


# ---- 3. many iterations and contention -----------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """One brain of 3 000 001 records over 100 512 neurons, uploaded once; the tests below only read it."""
    import abnn_amd

    syn = _records(BIG, 5, BIG_NRN)
    syn.setflags(write=False)
    b = abnn_amd.Brain(256, 256, 100_000, BIG, 100_000)
    b.upload_synapses(syn)
    yield b, syn
    b.close()


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("weights", [None, (0.5, 2.0)])
def test_big_uniform_graph(gpu, big, reverse, weights):
    b, syn = big
    got = _against_reference(b, (0, 1), 64, reverse, weights, syn=syn)
    assert got["records"] == BIG and got["neurons"] == BIG_NRN and got["complete"] == 1
    if not reverse and weights is None:
        assert got["levels"][:7].tolist() == [1, 36, 1079, 27348, 72027, 21, 0] and got["reached"] == BIG_NRN
    if weights is not None and not reverse:  # about half of the edges: one hop more
        assert got["depth"] == 6 and got["reached"] == BIG_NRN


def test_big_uniform_graph_other_seeds(gpu, big):
    b, syn = big
    _against_reference(b, (BIG_NRN - 1, 1), 3, syn=syn)            # cut off while the frontier is at its widest
    _against_reference(b, (256, 256), 64, reverse=True, syn=syn)
    _against_reference(b, (0, BIG_NRN), 2, syn=syn)                # every neuron a seed: one live step


# ---- 4. the recipe ---------------------------------------------------------------------------------------
def test_the_recipe_cannot_drive_the_hidden_block(gpu):
    with _brain(1_000_000, n_hidden=99_488) as b:
        b.build_random_graph(1)
        syn = b.download_synapses()
        fwd = _against_reference(b, (0, 256), 8, syn=syn)
        assert fwd["levels"].tolist() == [256, 256, 0, 0, 0, 0, 0, 0, 0]
        rev = _against_reference(b, (256, 256), 8, reverse=True, syn=syn)
        assert rev["levels"].tolist() == [256, 256, 0, 0, 0, 0, 0, 0, 0]
        assert (fwd["dist"][512:] == NONE).all() and (rev["dist"][512:] == NONE).all()
        hid = _against_reference(b, (512, 1), 64, syn=syn)
        assert hid["complete"] == 1 and hid["reached"] > 90_000 and (hid["dist"][:512] == NONE).all()


# ---- 5. high neuron ids ------------------------------------------------------------------------------------
def test_high_neuron_ids(gpu):
    import abnn_amd
    from abnn_amd import SYN_DTYPE

    n_nrn = (1 << 24) - 2  # the largest N_NRN; not a multiple of 4: the plane's and the bitmap's last word are partial
    last = n_nrn - 1
    edges = []
    for base in (1 << 16, 1 << 18, 1 << 23):
        edges += [(i, i + 1) for i in range(base - 3, base + 3)]
    edges += [(last - 2, last - 1), (last - 1, last), (last, 5), (5, 6), (6, (1 << 23) - 3), ((1 << 16) + 3, (1 << 18) - 3)]
    rng = np.random.default_rng(9)
    n_syn = 3001
    syn = np.zeros(n_syn, dtype=SYN_DTYPE)
    syn["src"] = rng.integers(0, n_nrn, n_syn, dtype=np.uint32)
    syn["dst"] = rng.integers(0, n_nrn, n_syn, dtype=np.uint32)
    syn["w"] = rng.uniform(0.0, 1.0, n_syn).astype(F32)
    at = rng.choice(n_syn, len(edges), replace=False)
    at[0] = n_syn - 1  # the record that no whole load holds
    for k, (s, d) in zip(at, edges):
        syn["src"][k], syn["dst"][k] = s, d
    with abnn_amd.Brain(256, 256, n_nrn - 512, n_syn, 100_000) as b:
        assert b.n_neuron() == n_nrn
        b.upload_synapses(syn)
        got = _against_reference(b, ((1 << 16) - 3, 1), 32, syn=syn)
        assert got["dist"][(1 << 16) + 3] == 6 and got["dist"][(1 << 18) + 3] == 13
        got = _against_reference(b, (last, 1), 32, syn=syn)          # the last valid id as a seed
        assert got["dist"][last] == 0 and got["dist"][5] == 1 and got["dist"][(1 << 23) + 3] == 9
        got = _against_reference(b, (last - 2, 1), 32, syn=syn)      # ... and as a target
        assert got["dist"][last] == 2
        got = _against_reference(b, (last, 1), 32, reverse=True, syn=syn)
        assert got["dist"][last - 2] == 2
        got = _against_reference(b, ((1 << 23) + 3, 1), 32, reverse=True, syn=syn)
        assert got["dist"][last] == 9 and got["dist"][last - 2] == 11
        _against_reference(b, (n_nrn - 40, 40), 2, weights=(0.0, 2.0), syn=syn)
        # more seeds than the LDS fold of the bitmap takes (csrc/hops.h kHopsFoldMaxFrontier) over a bitmap that
        # does not fit it: the expand kernel tests the bitmap itself
        from abnn_amd import hops

        assert 50_000 > hops.FOLD_MAX_FRONTIER and 40_000 > hops.FOLD_MAX_FRONTIER and n_nrn > 32 * hops.FOLD_WORDS
        for reverse in (False, True):
            got = _against_reference(b, (n_nrn - 50_000, 50_000), 3, reverse, syn=syn)
            assert got["levels"][0] == 50_000 and got["levels"][1] >= 2
        _against_reference(b, (0, 40_000), 2, weights=(0.5, 1.0), syn=syn)


# ---- 6. tombstones and headroom ------------------------------------------------------------------------------
def test_tombstones_and_capacity_headroom(gpu):
    syn = _records(5_000, 3)
    dead = np.random.default_rng(4).choice(5_000, 500, replace=False)
    syn["src"][dead] = NONE
    syn["dst"][dead] = NONE
    with _brain(5_000, syn_capacity=9_000) as b:
        b.upload_synapses(syn)
        back = b.download_synapses()
        assert int((back["dst"] == NONE).sum()) == 500
        for reverse in (False, True):
            got = _against_reference(b, (0, 1), 64, reverse, syn=back)
            assert got["records"] == 5_000
            _against_reference(b, (256, 256), 64, reverse, (0.25, 0.9), syn=back)
    with _brain(0) as b:  # no records: the seeds only
        got = b.hops((10, 5), 4)
        assert got["levels"].tolist() == [5, 0, 0, 0, 0] and got["reached"] == 5 and got["complete"] == 1
        assert got["records"] == 0 and (got["dist"][10:15] == 0).all() and int((got["dist"] == NONE).sum()) == 995


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
    before = _against_reference(b, (512, 1), 64, syn=syn)
    b.set_auto_stimulus(0, 256)
    b.encode_traversal(2)  # the second pass runs the structural update: the tombstones are removed
    assert b.n_syn() <= n_syn - 20_000
    after_syn = b.download_synapses()
    assert len(after_syn) == b.n_syn() and not (after_syn["dst"] == NONE).any()
    after = _against_reference(b, (512, 1), 64, syn=after_syn)
    assert after["records"] == b.n_syn() < before["records"]
    _against_reference(b, (256, 256), 64, reverse=True, syn=after_syn)
    _against_reference(b, (0, 256), 64, weights=(0.2, INF), syn=after_syn)
    b.close()


# ---- 7. the enqueue-only path ------------------------------------------------------------------------------
def test_enqueue_between_passes_on_a_side_stream(gpu):
    import torch

    import abnn_amd
    from abnn_amd import hops

    def make():
        b = abnn_amd.Brain(256, 256, 99_488, 1_000_000, 1_000_000)
        b.build_random_graph(1)
        b.set_auto_stimulus(0, 256)
        return b

    a, twin = make(), make()
    n_nrn = a.n_neuron()
    cfgs = [hops.config((512, 1), 64), hops.config((256, 256), 8, reverse=True, weights=(0.5, INF)),
            hops.config((512, 1), 64)]  # the first config again: the scratch is reused
    outs = [torch.zeros(hops.n_words(c, n_nrn), dtype=torch.int64, device="cuda:0") for c in cfgs]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=0)
    a.encode_traversal(6, stream=side)  # the weights move from the fourth pass
    for c, o in zip(cfgs, outs):
        a.hops_enqueue(c, o.data_ptr(), stream=side)
    a.encode_traversal(2, stream=side)
    side.synchronize()  # the only synchronise
    twin.encode_traversal(6)
    syn = twin.download_synapses()
    got = [hops.decode(o.cpu().numpy().view(np.uint64), c, n_nrn) for c, o in zip(cfgs, outs)]
    for c, g in zip(cfgs, got):
        _same(g, hops.reference(syn, c, n_nrn))
    assert np.array_equal(_words(got[0]), _words(got[2]))
    assert got[0]["reached"] > 1000 and got[1]["levels"][0] == 256
    twin.encode_traversal(2)
    assert a.checksum() == twin.checksum()  # the search wrote nothing but its result
    assert np.array_equal(a.download_synapses().view(np.uint32), twin.download_synapses().view(np.uint32))
    assert np.array_equal(a.last_fired(), twin.last_fired()) and a.scalars() == twin.scalars()
    assert a.stats() == twin.stats()
    # refused on the host, before any launch
    for bad in (hops.config((5, 0)), hops.config((n_nrn - 1, 2)), hops.config((0, 1), 0), hops.config((0, 1), 1025)):
        with pytest.raises(abnn_amd.AbnnError) as err:
            a.hops_enqueue(bad, outs[0].data_ptr())
        assert err.value.status == 1
    for step in (65, 1024, 0xFFFFFFFE):
        with pytest.raises(abnn_amd.AbnnError) as err:
            a.hops_step_enqueue(cfgs[0], step, outs[0].data_ptr())
        assert err.value.status == 1
    with pytest.raises(abnn_amd.AbnnError) as err:
        a.hops((0, 1), 64, weights=(0.5, 0.5))
    assert err.value.status == 1
    a.close()
    twin.close()


# ---- 8. steps and shards -------------------------------------------------------------------------------------
def test_stepped_shards_equal_the_unsharded_search(gpu):
    import torch

    import abnn_amd
    from abnn_amd import hops
    from abnn_amd.shard import global_events, shard_ranges

    n_syn, events = 10_000, 100_000
    with _brain(n_syn) as whole:
        syn = _records(n_syn, 7)
        whole.upload_synapses(syn)
        n_nrn = whole.n_neuron()
        ge = global_events(n_syn, events, 3)
        shards = []
        for lo, hi in shard_ranges(n_syn, 3):
            s = abnn_amd.Brain(256, 256, 488, hi - lo, events, syn_offset=lo, global_events=ge)
            s.upload_synapses(syn[lo:hi])
            shards.append(s)
        for args in (((0, 1), 16), ((256, 256), 16, True), ((700, 3), 5, False, (0.3, 0.9)), ((0, 1), 2)):
            cfg = hops.config(*args)
            want = _against_reference(whole, *args, syn=syn)
            at = hops.plane_offset(cfg)
            outs = [torch.zeros(hops.n_words(cfg, n_nrn), dtype=torch.int64, device="cuda:0") for _ in shards]
            for s, o in zip(shards, outs):
                s.hops_step_enqueue(cfg, hops.BEGIN, o.data_ptr())
            for h in range(cfg.max_hops + 1):
                for s, o in zip(shards, outs):
                    s.hops_step_enqueue(cfg, h, o.data_ptr())
                torch.cuda.synchronize()
                planes = [o[at:].cpu().numpy().view(np.uint32) for o in outs]
                merged = torch.from_numpy(hops.merge_planes(planes).view(np.int64)).to("cuda:0")
                for o in outs:
                    o[at:].copy_(merged)
            torch.cuda.synchronize()
            for (lo, hi), o in zip(shard_ranges(n_syn, 3), outs):
                got = hops.decode(o.cpu().numpy().view(np.uint64), cfg, n_nrn)
                assert got["records"] == hi - lo
                got["records"] = n_syn
                _same(got, want, str(args))
            alone = shards[0].hops(*args)
            if args == ((0, 1), 16):
                assert alone["reached"] < want["reached"]  # one shard holds only some of the edges
        for s in shards:
            s.close()


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_sharded_brain_hops_world1(gpu, monkeypatch):
    import torch.distributed as dist

    from abnn_amd.shard import ShardedBrain, TorchComm

    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(_port()))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        sb = ShardedBrain(TorchComm(), 256, 256, 488, 10_000, 100_000, device=0, native=True)
        sb.brain.build_random_graph(1)
        for args in (((0, 256), 8), ((256, 256), 8, True), ((512, 1), 64), ((512, 1), 3, False, (0.3, 0.9)), ((0, 1), 1)):
            _same(sb.hops(*args), _against_reference(sb.brain, *args), str(args))
        sb.native.close()
        sb.brain.close()
    finally:
        dist.destroy_process_group()


# ---- 9. the C++ mirrors ----------------------------------------------------------------------------------------
def test_cpp_hops(gpu):
    from abnn_amd.build import build_hops_test

    prog = build_hops_test()
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    lines = r.stdout.strip().splitlines()
    assert lines, (r.returncode, r.stderr[-2000:])
    res = json.loads(lines[-1])
    assert r.returncode == 0 and res["ok"], (res, r.stderr[-2000:])
    assert res["records"] == 100_000 and res["neurons"] == 10_000
    assert res["inputs_level0"] == 256 == res["inputs_level1"]
    assert res["hidden_reached"] > 1 and res["hidden_depth"] >= 1 and res["cut_complete"] == 0
