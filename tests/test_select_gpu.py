"""The synapse select on the GPU (abnn.h abnn_select_*, csrc/select.hip).

Every comparison is Brain.select (or select_enqueue into a prefilled torch
buffer) against select.reference over the same brain's download_synapses(),
all words up to `written` equal: record-count edges around the tile and the
vector tail, a brain of several tiles per CU, few workgroups that loop, a scan
of two segments, capacities that cut inside a tile and at a tile boundary,
degenerate layouts, the census and the degree
census on the same brain, the generated graph, tombstones and growth, capacity
headroom, the enqueue-only path on a side stream, shards, and the C++ mirrors."""
import json
import socket
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
NONE = 0xFFFFFFFF
INF = float("inf")
SPECIAL = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-40, 0.25, 0.75, 0.7499999, 0.25000003], dtype=F32)
BIG = 3_000_001  # 733 tiles over every CU; the last record is in no 16-byte pair
BIG_NRN = 100_512  # 256 + 256 + 100 000
USED_NRN = 100_000  # the seeded records of the big brain use the neurons below; the planted ones those above
SENTINEL = 0x5A5A5A5A5A5A5A5A


def _same(got, want, what=""):
    for k in ("records", "tombstones", "matched", "written", "syn_offset", "capacity"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert got["index"].dtype == np.uint64 and got["index"].shape == (want["written"],), what
    bad = np.flatnonzero(got["index"] != want["index"])
    assert bad.size == 0, (what, bad[:8].tolist(), got["index"][bad[:8]].tolist(), want["index"][bad[:8]].tolist())
    g, w = got["syn"].view(np.uint32).reshape(-1, 4), want["syn"].view(np.uint32).reshape(-1, 4)
    bad = np.flatnonzero((g != w).any(axis=1))
    assert bad.size == 0, (what, bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist())


def _against_reference(b, kw, capacity, syn=None, note=""):
    """Brain.select against the reference; capacity None = exactly the matches."""
    from abnn_amd import select

    syn = b.download_synapses() if syn is None else syn
    cfg = select.config(**kw)
    got = b.select(capacity=capacity, **kw)
    offset = int(b.dims.syn_offset)
    matched = int(select.matches(syn, cfg).sum())
    want = select.reference(syn, cfg, matched if capacity is None else capacity, b.n_neuron(), syn_offset=offset)
    _same(got, want, f"{note} {kw} capacity {capacity}")
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


def _brain(n_syn, **kw):
    import abnn_amd

    return abnn_amd.Brain(256, 256, 488, n_syn, 100_000, **kw)


def _big_brain():
    import abnn_amd

    return abnn_amd.Brain(256, 256, 100_000, BIG, 100_000)


def _tile():
    from abnn_amd import select

    return select.TILE


SMALL_CONFIGS = (dict(), dict(dst=(256, 256)), dict(src=(0, 500)), dict(src=(100, 600), dst=(300, 600)),
                 dict(src=(0, 100), dst=(900, 100), any=True), dict(dst=(999, 1), any=True),
                 dict(weights=(0.25, 0.75)), dict(src=(0, 500), weights=(0.25, INF)),
                 dict(src=(0, 300), dst=(0, 300), weights=(-INF, 0.25), any=True))


# ---- 1. record-count edges ---------------------------------------------------------------------
@pytest.mark.parametrize("tiles, more", [(0, 1), (0, 63), (0, 64), (0, 65), (1, -1), (1, 0), (1, 1), (2, 1), (0, 10_000)])
def test_record_count_edges(gpu, tiles, more):
    n_syn = tiles * _tile() + more
    with _brain(n_syn) as b:
        syn = _records(n_syn, 1)
        b.upload_synapses(syn)
        back = b.download_synapses()
        assert np.array_equal(back.view(np.uint32), syn.view(np.uint32))
        for kw in SMALL_CONFIGS:
            whole = _against_reference(b, kw, None, syn=back, note=f"n {n_syn}")
            assert whole["records"] == n_syn and whole["tombstones"] == 0 and whole["written"] == whole["matched"]
            m = whole["matched"]
            for cap in sorted({0, 1, max(m - 1, 0), m + 1}):
                _against_reference(b, kw, cap, syn=back, note=f"n {n_syn}")
        every = b.select()
        assert every["matched"] == n_syn and np.array_equal(every["index"], np.arange(n_syn, dtype=np.uint64))


# ---- 2. a brain of 733 tiles ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """One brain of 3 000 001 records over 100 512 neurons, uploaded once; the
    tests below only read it.  dst 100 500 is planted at the first and the last
    record only (as is src 100 400), dst 100 501 at every third record of the
    last tile only."""
    syn = _records(BIG, 5, USED_NRN)
    syn["dst"][[0, BIG - 1]] = 100_500
    last_tile = (BIG - 1) // _tile() * _tile()
    syn["dst"][last_tile + 1:BIG - 1:3] = 100_501
    syn["src"][[0, BIG - 1]] = 100_400
    syn.setflags(write=False)
    b = _big_brain()
    b.upload_synapses(syn)
    yield b, syn
    b.close()


def _enqueue(b, cfg, capacity):
    """select_enqueue into a torch buffer prefilled with SENTINEL: the words, and
    the entries of both planes past `written` must still hold it."""
    import torch

    from abnn_amd import select

    words = select.n_words(cfg, capacity)
    out = torch.full((words,), SENTINEL, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    b.select_enqueue(cfg, capacity, out.data_ptr())
    b.synchronize()
    torch.cuda.synchronize()
    w = out.cpu().numpy().view(np.uint64)
    n = int(w[3])
    assert n <= capacity
    assert (w[8 + n:8 + capacity] == SENTINEL).all(), "index plane written past `written`"
    assert (w[8 + capacity + 2 * n:] == SENTINEL).all(), "record plane written past `written`"
    w = w.copy()
    w[8 + n:8 + capacity] = 0
    w[8 + capacity + 2 * n:] = 0
    return select.decode(w, capacity)


def _big_cases():
    return {
        "no match": dict(dst=(100_510, 1)),
        "the first and the last record": dict(dst=(100_500, 1)),
        "the first and the last record by src": dict(src=(100_400, 1)),
        "the last tile only": dict(dst=(100_501, 1)),
        "half the records, by src": dict(src=(0, 50_000)),
        "a hidden window's neighbourhood": dict(src=(512, 4096), dst=(512, 4096), any=True),
        "at least 0.9": dict(weights=(0.9, INF)),
        "all three": dict(src=(0, 50_000), dst=(50_000, 50_000), weights=(0.25, 0.75)),
    }


@pytest.mark.parametrize("case", sorted(_big_cases()))
def test_big_brain(gpu, big, case):
    from abnn_amd import select

    b, syn = big
    tile = _tile()
    assert BIG > 700 * tile and BIG % 2 == 1
    kw = _big_cases()[case]
    cfg = select.config(**kw)
    mask = select.matches(syn, cfg)
    matched = int(mask.sum())
    # a capacity that ends exactly with a tile's matches, and one that cuts inside the next tile
    per_tile = np.add.reduceat(mask.astype(np.int64), np.arange(0, BIG, tile))
    cum = np.cumsum(per_tile)
    caps = {0, 1, matched, matched + 5}
    if matched > 4 * tile:
        t = len(per_tile) // 3
        assert per_tile[t + 1] > 7
        caps |= {int(cum[t]), int(cum[t]) + 7}
    for cap in sorted(caps):
        got = _enqueue(b, cfg, cap)
        _same(got, select.reference(syn, cfg, cap, BIG_NRN), f"{case} capacity {cap}")
        assert got["matched"] == matched and got["records"] == BIG
    if case == "no match":
        assert matched == 0
    if case.startswith("the first and the last record"):
        assert got["index"].tolist() == [0, BIG - 1]
    if case == "the last tile only":
        assert matched > 100 and int(got["index"].min()) > (BIG - 1) // tile * tile and int(got["index"].max()) < BIG - 1


def test_big_brain_every_record(gpu, big):
    from abnn_amd import select

    b, syn = big
    got = _enqueue(b, select.config(), BIG)
    assert got["written"] == got["matched"] == BIG and got["tombstones"] == 0
    assert np.array_equal(got["index"], np.arange(BIG, dtype=np.uint64))
    assert np.array_equal(got["syn"].view(np.uint32), syn.view(np.uint32))  # pad 0 on both sides
    assert _enqueue(b, select.config(), 0)["matched"] == BIG


def test_few_workgroups_loop_over_tiles_and_chunks(gpu, big, monkeypatch):
    """The count launch strides over the tiles and the emit launch over chunks of
    64 tiles only when there are more of them than workgroups: 3 workgroups
    (ABNN_SELECT_BLOCKS, read when the handle is created) over 733 tiles."""
    from abnn_amd import select

    _, syn = big
    monkeypatch.setenv("ABNN_SELECT_BLOCKS", "3")
    with _big_brain() as b:
        b.upload_synapses(syn)
        for kw in (dict(src=(0, 50_000)), dict(dst=(100_501, 1)), dict(weights=(0.9, INF)), dict()):
            cfg = select.config(**kw)
            matched = int(select.matches(syn, cfg).sum())
            for cap in (matched, matched // 2 + 3):
                _same(_enqueue(b, cfg, cap), select.reference(syn, cfg, cap, BIG_NRN), f"{kw} capacity {cap}")


def test_the_scan_carries_across_its_iterations(gpu):
    """k_select_scan takes 16 384 tile counts per iteration: 70 000 001 generated
    records are 17 090 tiles.  Too many to compare record by record in a quick
    test, so: matched equals the degree census's count, every returned record
    obeys the rule, the indices increase, and the records at the first, a
    middle and the last returned index are the brain's."""
    import abnn_amd

    n_syn = 70_000_001
    assert n_syn > 16_384 * _tile()
    with abnn_amd.Brain(256, 256, 99_488, n_syn, 100_000) as b:
        b.build_random_graph(1)
        for n in (600, 99_000):
            got = b.select(src=(n, 1), dst=(n, 1), any=True)
            deg = b.degrees((n, 1), ("out", "in"))
            s, d = got["syn"]["src"], got["syn"]["dst"]
            loops = int(((s == n) & (d == n)).sum())
            assert got["matched"] == got["written"] == int(deg["out"][0]) + int(deg["in"][0]) - loops > 1000
            assert ((s == n) | (d == n)).all() and (np.diff(got["index"].astype(np.int64)) > 0).all()
            assert int(got["index"][-1]) > 16_384 * _tile() and int(got["index"][-1]) < n_syn
            for k in (0, got["written"] // 2, got["written"] - 1):
                rec = b.download_synapses(int(got["index"][k]), 1)
                assert np.array_equal(rec.view(np.uint32), got["syn"][k:k + 1].view(np.uint32)), k
        every = b.select(capacity=0)
        assert every["matched"] == every["records"] == n_syn and every["tombstones"] == 0


# ---- 3. degenerate layouts ------------------------------------------------------------------------
def _degenerate(kind, base):
    syn = base.copy()
    rng = np.random.default_rng(11)
    if kind == "one pair":
        syn["src"], syn["dst"] = 7, 300
    elif kind == "src sorted":
        syn["src"] = np.sort(syn["src"])
    else:  # runs of 256
        syn["src"] = np.repeat(rng.integers(0, USED_NRN, BIG // 256 + 1, dtype=np.uint32), 256)[:BIG]
    return syn


@pytest.mark.parametrize("kind", ["one pair", "src sorted", "runs of 256"])
def test_degenerate_layouts(gpu, big, kind):
    _, base = big
    syn = _degenerate(kind, base)
    with _big_brain() as b:
        b.upload_synapses(syn)
        if kind == "one pair":
            for kw in (dict(src=(7, 1)), dict(dst=(300, 1)), dict(src=(7, 1), dst=(300, 1)),
                       dict(src=(8, 1), dst=(300, 1), any=True)):
                got = _against_reference(b, kw, 10_000, syn=syn, note=kind)
                assert got["matched"] == BIG and got["index"].tolist() == list(range(10_000))
            assert _against_reference(b, dict(src=(8, 1), dst=(300, 1)), 10, syn=syn, note=kind)["matched"] == 0
            assert _against_reference(b, dict(dst=(300, 1)), None, syn=syn, note=kind)["written"] == BIG
        else:
            for kw in (dict(src=(1000, 3000)), dict(src=(40_000, 1)), dict(src=(0, 20_000), weights=(0.0, 0.5)),
                       dict(src=(99_000, 1000), dst=(0, 1000), any=True)):
                got = _against_reference(b, kw, None, syn=syn, note=kind)
                _against_reference(b, kw, got["matched"] // 2 + 1, syn=syn, note=kind)


# ---- 4. the census and the degree census of the same brain ------------------------------------------
def test_cross_checks_against_census_and_degrees(gpu, big):
    b, syn = big
    for src, dst in ((None, (256, 256)), ((0, 50_000), None), ((512, 4096), (512, 4096)), ((100_400, 1), (100_500, 1))):
        matched = b.select(src=src, dst=dst, capacity=0)["matched"]
        assert matched == b.census(4, -1.0, 2.0, src=src, dst=dst)["selected"], (src, dst)
    for n in (0, 511, 512, 77_777, 100_400, 100_500, 100_501, BIG_NRN - 1):
        deg = b.degrees((n, 1), ("out", "in"))
        assert b.select(src=(n, 1), capacity=0)["matched"] == int(deg["out"][0]), n
        assert b.select(dst=(n, 1), capacity=0)["matched"] == int(deg["in"][0]), n
        both = b.select(src=(n, 1), dst=(n, 1), any=True)
        loops = int(((syn["src"] == n) & (syn["dst"] == n)).sum())
        assert both["matched"] == int(deg["out"][0]) + int(deg["in"][0]) - loops, n


# ---- 5. the generated graph ------------------------------------------------------------------------------
def test_the_generated_graph(gpu):
    import abnn_amd

    with _brain(100_000) as b:
        b.build_random_graph(1)
        syn = b.download_synapses()
        fields = _against_reference(b, dict(dst=(256, 256)), None, syn=syn)
        assert fields["matched"] == fields["written"] == 65_536
        assert (np.bincount(fields["syn"]["dst"] - 256, minlength=256) == 256).all()
        assert (fields["syn"]["src"] < 256).all()
        assert np.array_equal(fields["index"], np.arange(65_536, dtype=np.uint64))  # the dense block comes first
        _against_reference(b, dict(src=(0, 256)), None, syn=syn)
        _against_reference(b, dict(weights=(0.19, INF)), None, syn=syn)
        hidden = _against_reference(b, dict(src=(512, 488), dst=(512, 488)), None, syn=syn)
        assert hidden["matched"] == 100_000 - 65_536
        # the selected records as a smaller brain's records
        with _brain(fields["written"]) as small:
            small.upload_synapses(fields["syn"])
            back = small.download_synapses()
            assert np.array_equal(back.view(np.uint32), fields["syn"].view(np.uint32))
            assert small.checksum() != 0
        assert isinstance(fields["syn"], np.ndarray) and fields["syn"].dtype == abnn_amd.SYN_DTYPE


# ---- 6. tombstones and growth -------------------------------------------------------------------------
def test_tombstones_and_growth(gpu):
    import abnn_amd

    n_syn = 120_000
    b = abnn_amd.Brain(256, 256, 3000, n_syn, n_syn, syn_capacity=n_syn + 20_000, seed=13,
                       w_prune=0.105, p_new=0.35, w_init=0.5, compact_every=2)
    b.build_random_graph(21)
    b.set_auto_stimulus(0, 256)
    sizes, tombstones = set(), []
    for passes in range(1, 12, 2):
        b.encode_traversal(1)  # an odd number of passes: tombstones wait for the structural update
        syn = b.download_synapses()
        got = _against_reference(b, dict(), None, syn=syn, note=f"after pass {passes}")
        assert got["tombstones"] == int((syn["src"] == NONE).sum())
        tombstones.append(got["tombstones"])
        assert got["records"] == b.n_syn() and got["matched"] == b.n_syn() - got["tombstones"]
        _against_reference(b, dict(src=(512, 3000), weights=(0.0, 0.15)), None, syn=syn)
        b.encode_traversal(1)  # the structural update: tombstones removed, grown records appended
        syn = b.download_synapses()
        got = _against_reference(b, dict(), None, syn=syn, note=f"after pass {passes + 1}")
        assert got["tombstones"] == 0 and got["records"] == got["matched"] == b.n_syn() == len(syn)
        _against_reference(b, dict(dst=(512, 3000), weights=(0.5, 0.5000001)), None, syn=syn)  # the grown records
        sizes.add(b.n_syn())
    st = b.stats()
    assert max(tombstones) > 0, tombstones  # pruning starts once hidden neurons spike
    assert st["pruned"] > 0 and st["grown"] > 0 and sizes != {n_syn}
    b.close()


# ---- 7. capacity headroom ----------------------------------------------------------------------------------
def test_capacity_beyond_n_syn_is_not_selected(gpu):
    from abnn_amd import select

    syn = _records(5_000, 3)
    with _brain(5_000, syn_capacity=9_000) as b:
        b.upload_synapses(syn)
        for kw in (dict(), dict(dst=(256, 256)), dict(weights=(-INF, INF))):
            got = _against_reference(b, kw, 9_000, syn=syn)
            assert got["records"] == 5_000 and (got["index"] < 5_000).all()
        assert b.select()["matched"] == 5_000
    with _brain(0) as b:  # no records: a valid, all-zero header
        for kw in (dict(), dict(dst=(0, 256))):
            for cap in (0, 4):
                got = b.select(capacity=cap, **kw)
                assert not select.to_words(got).any() and got["written"] == 0


# ---- 8. the enqueue-only path ------------------------------------------------------------------------------
def test_enqueue_between_passes_on_a_side_stream(gpu):
    import torch

    import abnn_amd
    from abnn_amd import select

    def make():
        b = abnn_amd.Brain(256, 256, 99_488, 1_000_000, 1_000_000)
        b.build_random_graph(1)
        b.set_auto_stimulus(0, 256)
        return b

    a, twin = make(), make()
    jobs = [(dict(dst=(256, 256)), 70_000), (dict(weights=(0.19, INF)), 200_000), (dict(src=(0, 256), dst=(300, 8)), 100)]
    cfgs = [select.config(**kw) for kw, _ in jobs]
    outs = [torch.zeros(select.n_words(c, cap), dtype=torch.int64, device="cuda:0") for c, (_, cap) in zip(cfgs, jobs)]
    assert a.select(capacity=0)["matched"] == 1_000_000  # the first select allocates the handle's scratch
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=0)
    a.encode_traversal(6, stream=side)  # the weights move from the fourth pass
    for c, o, (_, cap) in zip(cfgs, outs, jobs):
        a.select_enqueue(c, cap, o.data_ptr(), stream=side)
    a.encode_traversal(2, stream=side)
    side.synchronize()  # the only synchronise
    twin.encode_traversal(6)
    syn = twin.download_synapses()
    for c, o, (kw, cap) in zip(cfgs, outs, jobs):
        got = select.decode(o.cpu().numpy().view(np.uint64), cap)
        want = twin.select(capacity=cap, **kw)
        _same(got, want, str(kw))
        _same(want, select.reference(syn, c, cap, a.n_neuron()), str(kw))
        assert got["matched"] > 0 and got["written"] == min(got["matched"], cap)
    with make() as fresh:
        first = fresh.select(dst=(256, 256))
    moved = twin.select(dst=(256, 256))
    # the passes before the select moved the weights
    assert not np.array_equal(first["syn"]["w"].view(np.uint32), moved["syn"]["w"].view(np.uint32))
    twin.encode_traversal(2)
    assert a.checksum() == twin.checksum()  # the select wrote nothing but its result
    assert np.array_equal(a.last_fired(), twin.last_fired()) and a.scalars() == twin.scalars()
    a.close()
    twin.close()


# ---- 9. shards ---------------------------------------------------------------------------------------------
def test_merge_of_three_shards_equals_the_unsharded_select(gpu):
    import abnn_amd
    from abnn_amd import select
    from abnn_amd.shard import global_events, shard_ranges

    n_syn, events = 10_000, 100_000
    with _brain(n_syn) as whole:
        whole.build_random_graph(1)
        syn = whole.download_synapses()
        syn["w"][[0, 3_333, 3_334, 9_999]] = [-0.0, -100.0, np.nan, 200.0]
        whole.upload_synapses(syn)
        ge = global_events(n_syn, events, 3)
        shards = []
        for lo, hi in shard_ranges(n_syn, 3):
            s = abnn_amd.Brain(256, 256, 488, hi - lo, events, syn_offset=lo, global_events=ge)
            s.upload_synapses(syn[lo:hi])
            shards.append(s)
        for kw in (dict(), dict(dst=(256, 256)), dict(src=(0, 20)), dict(src=(600, 50), dst=(600, 50), any=True),
                   dict(weights=(0.15, INF)), dict(weights=(-INF, 0.0))):
            matched = whole.select(capacity=0, **kw)["matched"]
            for cap in sorted({0, 1, matched // 2, matched, matched + 3}):
                parts = [s.select(capacity=cap, **kw) for s in shards]
                assert [p["records"] for p in parts] == [3334, 3333, 3333]
                assert [p["syn_offset"] for p in parts] == [0, 3334, 6667]
                _same(select.merge(parts, cap), _against_reference(whole, kw, cap, syn=syn), f"{kw} capacity {cap}")
        for s in shards:
            s.close()
        # one shard far into a graph: indices above 32 bits
        far = 5_000_000_000
        with abnn_amd.Brain(256, 256, 488, 3_333, events, syn_offset=far, global_events=ge) as s:
            s.upload_synapses(syn[3_334:6_667])
            got = _against_reference(s, dict(src=(14, 5)), None, syn=syn[3_334:6_667])  # records 3584 .. 4863
            assert got["syn_offset"] == far and got["matched"] > 0 and int(got["index"].min()) >= far
            assert int(got["index"].max()) < far + 3_333


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_sharded_brain_select_world1(gpu, monkeypatch):
    import torch.distributed as dist

    from abnn_amd import select
    from abnn_amd.shard import ShardedBrain, TorchComm

    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(_port()))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        sb = ShardedBrain(TorchComm(), 256, 256, 488, 10_000, 100_000, device=0, native=True)
        sb.brain.build_random_graph(1)
        syn = sb.brain.download_synapses()
        for kw, cap in ((dict(), None), (dict(dst=(256, 256)), None), (dict(src=(0, 30)), 100), (dict(dst=(999, 1)), 0),
                        (dict(src=(600, 50), dst=(600, 50), any=True, weights=(0.12, 0.18)), None)):
            cfg = select.config(**kw)
            n = int(select.matches(syn, cfg).sum()) if cap is None else cap
            _same(sb.select(capacity=cap, **kw), select.reference(syn, cfg, n, 1000), str((kw, cap)))
        sb.native.close()
        sb.brain.close()
    finally:
        dist.destroy_process_group()


# ---- 10. error statuses ----------------------------------------------------------------------------------
def test_error_statuses(gpu):
    import torch

    import abnn_amd
    from abnn_amd import select

    out = torch.zeros(8 + 3 * 4, dtype=torch.int64, device="cuda:0")
    with _brain(1_000) as b:
        b.build_random_graph(1)
        bad_flag = select.config(dst=(0, 4))
        bad_flag.flags = 8
        for cfg in (select.config(src=(900, 101)), select.config(dst=(1000, 1)), select.config(any=True), bad_flag):
            with pytest.raises(abnn_amd.AbnnError) as err:
                b.select_enqueue(cfg, 4, out.data_ptr())
            assert err.value.status == 1
        for kw in (dict(src=(900, 101)), dict(any=True), dict(weights=(0.5, 0.5))):
            with pytest.raises(abnn_amd.AbnnError) as err:
                b.select(**kw)
            assert err.value.status == 1, kw
        torch.cuda.synchronize()
        assert not out.cpu().numpy().any()  # a refused select writes nothing
        assert b.select(src=(900, 100), capacity=0)["records"] == 1_000


# ---- 11. the C++ mirrors ----------------------------------------------------------------------------------------
def test_cpp_select(gpu):
    from abnn_amd.build import build_select_test

    prog = build_select_test()
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    lines = r.stdout.strip().splitlines()
    assert lines, (r.returncode, r.stderr[-2000:])
    res = json.loads(lines[-1])
    assert r.returncode == 0 and res["ok"], (res, r.stderr[-2000:])
    assert res["records"] == 100_001 == res["everything"] and res["receptive_fields"] == 65_536
