"""The synapse census on the GPU (abnn.h abnn_census_*, csrc/census.hip).

Every comparison is Brain.census against census.reference over the same
brain's download_synapses(), all result words equal: record-count edges and
the vector tail, degenerate weight distributions, the src / dst ranges,
tombstones and growth, the enqueue-only path on a side stream, the hook inside
the device-resident learning loop, shards, and the C++ mirrors."""
import json
import socket
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
NONE = 0xFFFFFFFF
BINS = (1, 7, 64, 4096)
# the edge values of tests/test_census_abi.py for lo = 0, hi = 1
EDGES = np.array([0.0, np.nextafter(F32(1), F32(0)), 1.0, -0.25, np.inf, -np.inf, np.nan, -0.0], dtype=F32)
BIG = 3_000_001  # every workgroup loops more than once; the last record is in no 16-byte pair


def _words(d):
    from abnn_amd import census

    return census.to_words(d)


def _same(got, want, what=""):
    g, w = _words(got), _words(want)
    assert g.shape == w.shape, what
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (what, bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist())
    assert got["selected"] == got["under"] + got["over"] + got["nan"] + int(got["counts"].sum()), what


def _against_reference(b, bins, lo, hi, src=None, dst=None, syn=None, what=""):
    from abnn_amd import census

    syn = b.download_synapses() if syn is None else syn
    got = b.census(bins, lo, hi, src, dst)
    _same(got, census.reference(syn, census.config(bins, lo, hi, src, dst)), what)
    return got


def _records(n, seed, n_nrn=1000):
    """Seeded records with weights in [-0.1, 1.1] and the edge values planted
    at the first, a middle and the last index (all eight at each where they
    fit, else one each, rotated by the seed)."""
    from abnn_amd import SYN_DTYPE

    rng = np.random.default_rng(seed)
    syn = np.zeros(n, dtype=SYN_DTYPE)
    syn["src"] = rng.integers(0, n_nrn, n, dtype=np.uint32)
    syn["dst"] = rng.integers(0, n_nrn, n, dtype=np.uint32)
    syn["w"] = rng.uniform(-0.1, 1.1, n).astype(F32)
    k = len(EDGES)
    if n >= 3 * k:
        for at in (0, n // 2 - k // 2, n - k):
            syn["w"][at:at + k] = EDGES
    else:
        for j, at in enumerate(sorted({0, n // 2, n - 1})):
            syn["w"][at] = EDGES[(seed + j) % k]
    return syn


def _brain(n_syn, **kw):
    import abnn_amd

    return abnn_amd.Brain(256, 256, 488, n_syn, 100_000, **kw)


# ---- 1. record-count edges ---------------------------------------------------------------------
# 4096 records are one workgroup iteration (2 x 512 threads x 4 loads): 4095 .. 4097 cross it with and without
# the odd last record, 8193 is two iterations and that record
@pytest.mark.parametrize("n_syn", [1, 63, 64, 65, 255, 257, 2047, 2049, 10_000, 2, 3, 4095, 4096, 4097, 8193])
def test_record_count_edges(gpu, n_syn):
    planted = set()
    with _brain(n_syn) as b:
        # below 24 records one edge value per position: the seeds rotate all eight through
        for seed in range(8 if n_syn < 3 * len(EDGES) else 1):
            syn = _records(n_syn, seed)
            planted |= set(syn["w"].view(np.uint32).tolist())
            b.upload_synapses(syn)
            back = b.download_synapses()
            assert np.array_equal(back.view(np.uint32), syn.view(np.uint32))
            for bins in BINS:
                got = _against_reference(b, bins, 0.0, 1.0, syn=back, what=f"n {n_syn} bins {bins} seed {seed}")
                assert got["records"] == n_syn and got["selected"] == n_syn and got["tombstones"] == 0
            _against_reference(b, 64, -0.1, 1.1, syn=back, what=f"n {n_syn} wide")
            # the instance that reads the src streams
            ranged = _against_reference(b, 64, 0.0, 1.0, src=(0, 500), syn=back, what=f"n {n_syn} src range")
            assert ranged["selected"] == int((back["src"] < 500).sum())
    assert planted >= set(EDGES.view(np.uint32).tolist())


@pytest.fixture(scope="module")
def big():
    """One brain of 3 000 001 records, uploaded once; the tests below only read it."""
    syn = _records(BIG, 5)
    syn.setflags(write=False)
    b = _brain(BIG)
    b.upload_synapses(syn)
    yield b, syn
    b.close()


@pytest.mark.parametrize("bins", BINS)
def test_three_million_and_one_records(gpu, big, bins):
    b, syn = big
    got = _against_reference(b, bins, 0.0, 1.0, syn=syn, what=f"bins {bins}")
    assert got["records"] == BIG and got["nan"] == 3 and got["under"] > 6 and got["over"] > 6
    assert np.isneginf(got["min"]) and np.isposinf(got["max"])


def test_three_million_and_one_records_with_ranges(gpu, big):
    b, syn = big
    got = _against_reference(b, 64, 0.0, 1.0, src=(0, 500), dst=(250, 500), syn=syn)
    assert 0 < got["selected"] < BIG // 2
    _against_reference(b, 4096, -0.1, 1.1, src=(999, 1), syn=syn)
    _against_reference(b, 7, 0.0, 1.0, dst=(0, 1), syn=syn)


def test_capacity_beyond_n_syn_is_not_counted(gpu):
    syn = _records(5_000, 3)
    with _brain(5_000, syn_capacity=9_000) as b:
        b.upload_synapses(syn)
        for bins in BINS:
            got = _against_reference(b, bins, 0.0, 1.0, syn=syn)
            assert got["records"] == 5_000 == got["selected"]
    with _brain(0) as b:  # no records: a valid, empty result
        got = b.census(64, 0.0, 1.0)
        assert got["records"] == 0 and got["selected"] == 0 and int(got["counts"].sum()) == 0
        assert np.isposinf(got["min"]) and np.isneginf(got["max"])


# ---- 2. degenerate distributions ---------------------------------------------------------------
@pytest.mark.parametrize("kind", ["all equal", "one bin, distinct"])
def test_degenerate_distributions(gpu, big, kind):
    _, base = big
    syn = base.copy()
    if kind == "all equal":
        syn["w"] = F32(0.15)
    else:  # distinct values inside bin 2048 of 4096 (and bin 32 of 64) over [0, 1)
        syn["w"] = F32(0.5) + (np.arange(BIG, dtype=np.uint32) % 2000).astype(F32) * F32(2.0 ** -24)
    with _brain(BIG) as b:
        b.upload_synapses(syn)
        for bins in BINS:
            got = _against_reference(b, bins, 0.0, 1.0, syn=syn, what=f"{kind} bins {bins}")
            assert int(got["counts"].max()) == BIG and np.count_nonzero(got["counts"]) == 1
        if kind == "all equal":
            assert got["min"] == got["max"] == F32(0.15)


# ---- 3. ranges on the generated graph --------------------------------------------------------------
@pytest.mark.parametrize("n_syn", [10_000, 100_000])
def test_ranges_on_the_generated_graph(gpu, n_syn):
    """build_random_graph(1) on config 1's neurons.  Config 1 itself holds 10 000
    records, all inside the 256 x 256 input->output block; with 100 000 the
    whole block (65 536 records, weights in [0.4, 0.8)) and hidden mass exist."""
    dense = min(n_syn, 65_536)
    with _brain(n_syn) as b:
        b.build_random_graph(1)
        syn = b.download_synapses()
        got = _against_reference(b, 64, 0.0, 1.0, src=(0, 256), dst=(256, 256), syn=syn)
        assert got["selected"] == dense and got["under"] == got["over"] == got["nan"] == 0
        assert F32(0.4) <= got["min"] <= got["max"] < F32(0.8)
        assert int(got["counts"][25:52].sum()) == dense
        whole = _against_reference(b, 64, 0.0, 1.0, syn=syn)
        assert whole["selected"] == n_syn
        if n_syn > dense:
            assert int(whole["counts"][6:13].sum()) == n_syn - dense  # the hidden mass: U(0.1, 0.2)
        for src, dst in (((0, 256), None), ((10, 20), None), ((512, 100), None),      # src only
                         (None, (256, 256)), (None, (300, 10)), (None, (999, 1))):    # dst only
            for bins in (7, 4096):
                _against_reference(b, bins, 0.0, 1.0, src=src, dst=dst, syn=syn, what=f"{src} {dst} {bins}")
        empty = _against_reference(b, 64, 0.0, 1.0, src=(0, 256), dst=(0, 256), syn=syn)
        assert empty["selected"] == 0 and np.isposinf(empty["min"]) and np.isneginf(empty["max"])
        assert empty["records"] == n_syn
        import abnn_amd

        with pytest.raises(abnn_amd.AbnnError) as err:  # a range that ends above N_NRN
            b.census(64, 0.0, 1.0, src=(900, 101))
        assert err.value.status == 1
        with pytest.raises(abnn_amd.AbnnError) as err:
            b.census(0, 0.0, 1.0)
        assert err.value.status == 1


# ---- 4. tombstones and growth -------------------------------------------------------------------------
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
        got = _against_reference(b, 64, 0.0, 1.0, syn=syn, what=f"after pass {passes}")
        assert got["tombstones"] == int((syn["src"] == NONE).sum())
        tombstones.append(got["tombstones"])
        assert got["records"] == b.n_syn() and got["live"] == b.n_syn() - got["tombstones"]
        _against_reference(b, 4096, 0.0, 1.0, dst=(256, 256), syn=syn)
        b.encode_traversal(1)  # the structural update: tombstones removed, grown records appended
        syn = b.download_synapses()
        got = _against_reference(b, 64, 0.0, 1.0, syn=syn, what=f"after pass {passes + 1}")
        assert got["tombstones"] == 0 and got["records"] == b.n_syn() == len(syn)
        sizes.add(b.n_syn())
    st = b.stats()
    assert max(tombstones) > 0, tombstones  # pruning starts once hidden neurons spike
    assert st["pruned"] > 0 and st["grown"] > 0 and sizes != {n_syn}
    b.close()


# ---- 5. the enqueue-only path ------------------------------------------------------------------------------
def test_enqueue_between_passes_on_a_side_stream(gpu):
    import torch

    import abnn_amd
    from abnn_amd import census

    def make():
        b = abnn_amd.Brain(256, 256, 99_488, 1_000_000, 1_000_000)
        b.build_random_graph(1)
        b.set_auto_stimulus(0, 256)
        return b

    cfg = census.config(4096, 0.0, 1.0)
    a, twin = make(), make()
    out = torch.zeros(census.n_words(cfg), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=0)
    a.encode_traversal(6, stream=side)  # the weights move from the fourth pass
    a.census_enqueue(cfg, out.data_ptr(), stream=side)
    a.encode_traversal(2, stream=side)
    side.synchronize()  # the only synchronise
    got = census.decode(out.cpu().numpy().view(np.uint64), cfg)
    twin.encode_traversal(6)
    want = twin.census(4096, 0.0, 1.0)
    _same(got, want)
    _same(want, census.reference(twin.download_synapses(), cfg))
    with make() as fresh:
        first = fresh.census(4096, 0.0, 1.0)
    assert not np.array_equal(_words(first), _words(want))  # the passes before the census moved the weights
    twin.encode_traversal(2)
    assert a.checksum() == twin.checksum()  # the census wrote nothing but its result
    assert np.array_equal(a.last_fired(), twin.last_fired()) and a.scalars() == twin.scalars()
    bad = census.config(64, 1.0, 0.0)
    with pytest.raises(abnn_amd.AbnnError) as err:
        a.census_enqueue(bad, out.data_ptr())
    assert err.value.status == 1
    a.close()
    twin.close()


# ---- 6. inside the learning loop ---------------------------------------------------------------------------
def test_census_inside_the_learning_loop(gpu):
    import abnn_amd
    from test_learn_gpu import _brain as config1_brain
    from test_learn_gpu import _stimulus

    xin, xex = _stimulus(60)
    a, twin = config1_brain(), config1_brain()
    with abnn_amd.LearnEngine(a, win_size=25) as e, abnn_amd.LearnEngine(twin, win_size=25) as t:
        assert e.census_count() == 0
        e.set_census(64, 0.0, 1.0, every=20, capacity=2)
        e.run(xin, xex)
        assert e.census_count() == 3  # host-side, before anything synchronised
        steps, snaps = e.census_trace(1, 2)
        assert steps.tolist() == [40, 60]
        for first, n in ((0, 1), (0, 3), (3, 1), (2, 2)):  # evicted, evicted, not taken yet, past the end
            with pytest.raises(abnn_amd.AbnnError) as err:
                e.census_trace(first, n)
            assert err.value.status == 1, (first, n)
        # the twin without a census, stopped at the same steps
        t.run(xin[:40], xex[:40])
        _same(snaps[0], twin.census(64, 0.0, 1.0), "step 40")
        t.run(xin[40:], xex[40:])
        _same(snaps[1], _against_reference(twin, 64, 0.0, 1.0), "step 60")
        assert not np.array_equal(_words(snaps[0]), _words(snaps[1]))
        # the census left the trajectory alone
        assert a.checksum() == twin.checksum() and a.scalars() == twin.scalars()
        assert np.array_equal(a.last_fired(), twin.last_fired())
        (o1, s1), (o2, s2) = e.trace(0, 60), t.trace(0, 60)
        assert np.array_equal(o1, o2) and np.array_equal(s1.view(np.uint32), s2.view(np.uint32))
        assert e.state() == t.state()
        e.set_census(None)  # off: nothing more is taken, nothing is readable
        assert e.census_count() == 0
        e.run(xin[:20], xex[:20])
        assert e.census_count() == 0
        with pytest.raises(abnn_amd.AbnnError):
            e.census_trace(0, 1)
        with pytest.raises(abnn_amd.AbnnError) as err:
            e.set_census(64, 0.0, 1.0, every=0, capacity=2)
        assert err.value.status == 1
    a.close()
    twin.close()


# ---- 7. shards ---------------------------------------------------------------------------------------------
def test_merge_of_three_shards_equals_the_unsharded_census(gpu):
    import abnn_amd
    from abnn_amd import census
    from abnn_amd.shard import global_events, shard_ranges

    n_syn, events = 10_000, 100_000
    with _brain(n_syn) as whole:
        whole.build_random_graph(1)
        syn = whole.download_synapses()
        syn["w"][[0, 3_333, 3_334, 9_999]] = [-0.0, 0.0, np.nan, 2.0]  # something for min / max / NaN to merge
        whole.upload_synapses(syn)
        ge = global_events(n_syn, events, 3)
        shards = []
        for lo, hi in shard_ranges(n_syn, 3):
            s = abnn_amd.Brain(256, 256, 488, hi - lo, events, syn_offset=lo, global_events=ge)
            s.upload_synapses(syn[lo:hi])
            shards.append(s)
        for args in ((64, 0.0, 1.0, None, None), (4096, 0.0, 1.0, (0, 20), None), (7, 0.5, 0.7, None, (256, 100)),
                     (64, 0.0, 1.0, (0, 1), (256, 1))):
            parts = [s.census(*args) for s in shards]
            assert [p["records"] for p in parts] == [3334, 3333, 3333]
            _same(census.merge(parts), _against_reference(whole, *args, syn=syn), str(args))
        for s in shards:
            s.close()


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_sharded_brain_census_world1(gpu, monkeypatch):
    import torch.distributed as dist

    from abnn_amd.shard import ShardedBrain, TorchComm

    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(_port()))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        sb = ShardedBrain(TorchComm(), 256, 256, 488, 10_000, 100_000, device=0, native=True)
        sb.brain.build_random_graph(1)
        for args in ((64, 0.0, 1.0, None, None), (4096, 0.4, 0.8, (0, 30), (256, 256)), (7, 0.0, 1.0, (600, 10), None)):
            _same(sb.census(*args), _against_reference(sb.brain, *args), str(args))
        sb.native.close()
        sb.brain.close()
    finally:
        dist.destroy_process_group()


# ---- 8. the C++ mirrors ----------------------------------------------------------------------------------------
def test_cpp_census(gpu):
    from abnn_amd.build import build_census_test

    prog = build_census_test()
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    lines = r.stdout.strip().splitlines()
    assert lines, (r.returncode, r.stderr[-2000:])
    res = json.loads(lines[-1])
    assert r.returncode == 0 and res["ok"], (res, r.stderr[-2000:])
    assert res["records"] == 10_000 and res["dense_selected"] == 10_000
    assert res["snapshots"] == 2 and (res["step0"], res["step1"]) == (40, 60) and res["moved"] is True
