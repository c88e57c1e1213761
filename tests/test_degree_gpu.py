"""The neuron degree census on the GPU (abnn.h abnn_degree_*, csrc/degree.hip).

Every comparison is Brain.degrees against degree.reference over the same
brain's download_synapses(), all result words equal: record-count edges and
the vector tail, both paths and the sizes around their crossover, degenerate
key distributions (the wave aggregation), the generated graph, tombstones and
growth, capacity headroom, the enqueue-only path on a side stream, shards, and
the C++ mirrors."""
import json
import socket
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
NONE = 0xFFFFFFFF
# the special weights of tests/test_degree_abi.py
SPECIAL = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-40, 127.99999, 128.0, -128.0, -127.99999, 0.001, 2.0 ** -24,
                    2.0 ** -25, -(2.0 ** -24)], dtype=F32)
WHATS = (1, 2, 4, 8, 3, 12, 15)
BIG = 3_000_001  # every workgroup loops more than once; the last record is in no 16-byte pair
BIG_NRN = 100_512  # 256 + 256 + 100 000: the planes of every neuron cannot fit LDS


def _words(d):
    from abnn_amd import degree

    return degree.to_words(d)


def _same(got, want, what=""):
    g, w = _words(got), _words(want)
    assert g.shape == w.shape, what
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (what, bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist())
    if "out" in got:
        assert got["out_total"] == int(got["out"].sum()), what
    if "in" in got:
        assert got["in_total"] == int(got["in"].sum()), what


def _against_reference(b, neurons, what, syn=None, note=""):
    from abnn_amd import degree

    syn = b.download_synapses() if syn is None else syn
    got = b.degrees(neurons, what)
    _same(got, degree.reference(syn, degree.config(neurons, what), b.n_neuron()), f"{note} R {neurons} what {what}")
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


# ---- 1. record-count edges ---------------------------------------------------------------------
# 4096 records are one workgroup iteration (2 x 512 threads x 4 loads): 4095 .. 4097 cross it with and without
# the odd last record, 8193 is two iterations and that record
@pytest.mark.parametrize("n_syn", [1, 63, 64, 65, 255, 257, 2047, 2049, 10_000, 2, 3, 4095, 4096, 4097, 8193])
def test_record_count_edges(gpu, n_syn):
    planted = set()
    with _brain(n_syn) as b:
        # below 39 records one special value per position: the seeds rotate all of them through
        for seed in range(len(SPECIAL) if n_syn < 3 * len(SPECIAL) else 1):
            syn = _records(n_syn, seed)
            planted |= set(syn["w"].view(np.uint32).tolist())
            b.upload_synapses(syn)
            back = b.download_synapses()
            assert np.array_equal(back.view(np.uint32), syn.view(np.uint32))
            for neurons in (None, (0, 1), (999, 1), (256, 256)):
                for what in WHATS:
                    got = _against_reference(b, neurons, what, syn=back, note=f"n {n_syn} seed {seed}")
                    assert got["records"] == n_syn and got["tombstones"] == 0
            whole = b.degrees()
            assert whole["out_total"] == whole["in_total"] == n_syn
    assert planted >= set(SPECIAL.view(np.uint32).tolist())


@pytest.mark.parametrize("repeats", [True, False])
def test_the_odd_record_after_a_whole_iteration(gpu, repeats):
    """4097 records: the last one is alone in the second workgroup iteration, the only record of its lane, beside
    an absent second record; every other lane of that iteration holds none.  It repeats the src and dst of record
    4095 or shares neither, so its one add lands on a neuron that the first iteration also counted, or on one of
    its own.  (Record 4095 is in another iteration: no shuffle of scatter() sees the two side by side.)"""
    n_syn = 4097
    syn = _records(n_syn, 11)
    src, dst = int(syn["src"][4095]), int(syn["dst"][4095])
    syn["src"][4094] = syn["src"][4096] = src if repeats else (src + 1) % 1000
    syn["dst"][4094] = syn["dst"][4096] = dst if repeats else (dst + 1) % 1000
    with _brain(n_syn) as b:
        b.upload_synapses(syn)
        for neurons in (None, (src, 2) if src < 999 else (998, 2), (dst, 1)):
            for what in WHATS:
                got = _against_reference(b, neurons, what, syn=syn, note=f"repeats {repeats}")
                assert got["records"] == n_syn and got["tombstones"] == 0


# ---- 2. both paths and the boundary ----------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """One brain of 3 000 001 records over 100 512 neurons, uploaded once; the tests below only read it."""
    syn = _records(BIG, 5, BIG_NRN)
    syn.setflags(write=False)
    b = _big_brain()
    b.upload_synapses(syn)
    yield b, syn
    b.close()


def _crossover_sizes():
    from abnn_amd import degree

    one_scan = degree.NARROW_LDS_BYTES // 24  # the longest range whose four planes one narrow scan holds
    return [one_scan, one_scan + 1, degree.NARROW_MAX - 1, degree.NARROW_MAX, degree.NARROW_MAX + 1]


@pytest.mark.parametrize("what", [15, 1, 2, 4, 8])
def test_wide_path_every_neuron(gpu, big, what):
    from abnn_amd import degree

    b, syn = big
    assert BIG_NRN > degree.NARROW_MAX
    got = _against_reference(b, None, what, syn=syn)
    assert got["records"] == BIG and got["count"] == BIG_NRN
    if what == 15:
        assert got["out_total"] == got["in_total"] == BIG
        assert got["out_skipped"] == got["in_skipped"] == 3 * 5  # NaN, +-inf, +-128 at three places


@pytest.mark.parametrize("neurons", [(256, 256), (512, 4096), (50_000, 1)])
@pytest.mark.parametrize("what", [15, 2, 4])
def test_narrow_path(gpu, big, neurons, what):
    from abnn_amd import degree

    b, syn = big
    assert neurons[1] <= degree.NARROW_MAX
    got = _against_reference(b, neurons, what, syn=syn)
    assert got["first"] == neurons[0] and got["count"] == neurons[1]


@pytest.mark.parametrize("what", [15, 8, 1])
def test_sizes_around_the_crossover(gpu, big, what):
    b, syn = big
    for size in _crossover_sizes():
        for first in (0, BIG_NRN - size):
            _against_reference(b, (first, size), what, syn=syn)


# ---- 3. degenerate distributions ---------------------------------------------------------------------
def _degenerate(kind, base):
    syn = base.copy()
    rng = np.random.default_rng(11)
    if kind == "one pair":
        syn["src"], syn["dst"] = 7, 300
    elif kind == "src sorted":
        syn["src"] = np.sort(syn["src"])
    elif kind == "runs of 256":
        syn["src"] = np.repeat(rng.integers(0, BIG_NRN, BIG // 256 + 1, dtype=np.uint32), 256)[:BIG]
    else:  # negative strengths
        syn["w"] = F32(-0.5)
    return syn


@pytest.mark.parametrize("kind", ["one pair", "src sorted", "runs of 256", "all weights -0.5"])
def test_degenerate_distributions(gpu, big, kind):
    from abnn_amd import degree

    _, base = big
    syn = _degenerate(kind, base)
    with _big_brain() as b:
        b.upload_synapses(syn)
        wide = _against_reference(b, None, 15, syn=syn, note=kind)  # the wide path
        for neurons in ((0, 512), (0, degree.NARROW_MAX)):          # the narrow path, one scan and two
            narrow = _against_reference(b, neurons, 15, syn=syn, note=kind)
        _against_reference(b, (7, 1), 5, syn=syn, note=kind)
        _against_reference(b, (300, 1), 10, syn=syn, note=kind)
        if kind == "one pair":
            assert wide["out"][7] == BIG == wide["in"][300] == narrow["out"][7] == narrow["in"][300]
            assert int(wide["out"].sum()) == BIG and np.count_nonzero(wide["in"]) == 1
        if kind == "all weights -0.5":
            assert wide["out_skipped"] == 0 and int(wide["in_w"].sum()) == -BIG * (1 << 23)
            assert (wide["out_w"] == -(wide["out"].astype(np.int64) << 23)).all()


# ---- 4. the generated graph ------------------------------------------------------------------------------
def test_the_generated_graph(gpu):
    with _brain(100_000) as b:
        b.build_random_graph(1)
        syn = b.download_synapses()
        whole = _against_reference(b, None, 15, syn=syn)
        assert (whole["out"][:256] == 256).all() and (whole["in"][:256] == 0).all()  # the inputs
        outs = _against_reference(b, (256, 256), ("in", "in_w"), syn=syn)
        assert (outs["in"] == 256).all()
        strength = outs["in_w"] / float(1 << 24)
        assert (strength >= 256 * 0.4).all() and (strength < 256 * 0.8).all()
        ins = _against_reference(b, (0, 256), ("out", "out_w"), syn=syn)
        assert (ins["out"] == 256).all() and ins["out_total"] == 65_536 and ins["out_skipped"] == 0
        hidden = _against_reference(b, (512, 488), 15, syn=syn)
        assert hidden["out_total"] == hidden["in_total"] == 100_000 - 65_536
        import abnn_amd

        for neurons, what in (((900, 101), 15), ((5, 0), 15), (None, 0), (None, 16)):
            with pytest.raises(abnn_amd.AbnnError) as err:
                b.degrees(neurons, what)
            assert err.value.status == 1, (neurons, what)


# ---- 5. tombstones and growth -------------------------------------------------------------------------
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
        got = _against_reference(b, None, 15, syn=syn, note=f"after pass {passes}")
        assert got["tombstones"] == int((syn["src"] == NONE).sum())
        tombstones.append(got["tombstones"])
        assert got["records"] == b.n_syn()
        assert got["out_total"] == got["in_total"] == b.n_syn() - got["tombstones"]
        _against_reference(b, (256, 256), ("in", "in_w"), syn=syn)
        b.encode_traversal(1)  # the structural update: tombstones removed, grown records appended
        syn = b.download_synapses()
        got = _against_reference(b, None, 15, syn=syn, note=f"after pass {passes + 1}")
        assert got["tombstones"] == 0 and got["records"] == b.n_syn() == len(syn)
        assert got["out_total"] == got["in_total"] == b.n_syn()
        _against_reference(b, (512, 3000), 15, syn=syn)
        sizes.add(b.n_syn())
    st = b.stats()
    assert max(tombstones) > 0, tombstones  # pruning starts once hidden neurons spike
    assert st["pruned"] > 0 and st["grown"] > 0 and sizes != {n_syn}
    b.close()


# ---- 6. capacity headroom ----------------------------------------------------------------------------------
def test_capacity_beyond_n_syn_is_not_counted(gpu):
    syn = _records(5_000, 3)
    with _brain(5_000, syn_capacity=9_000) as b:
        b.upload_synapses(syn)
        for neurons in (None, (256, 256)):
            got = _against_reference(b, neurons, 15, syn=syn)
            assert got["records"] == 5_000
        assert b.degrees()["out_total"] == 5_000
    with _brain(0) as b:  # no records: a valid, all-zero result
        for neurons in (None, (0, 256)):
            got = b.degrees(neurons)
            assert not _words(got).any() and got["count"] == (256 if neurons else 1000)


# ---- 7. the enqueue-only path ------------------------------------------------------------------------------
def test_enqueue_between_passes_on_a_side_stream(gpu):
    import torch

    import abnn_amd
    from abnn_amd import degree

    def make():
        b = abnn_amd.Brain(256, 256, 99_488, 1_000_000, 1_000_000)
        b.build_random_graph(1)
        b.set_auto_stimulus(0, 256)
        return b

    a, twin = make(), make()
    n_nrn = a.n_neuron()
    cfgs = [degree.config(None, 15), degree.config((256, 256), ("in", "in_w"))]  # wide, narrow
    outs = [torch.zeros(degree.n_words(c, n_nrn), dtype=torch.int64, device="cuda:0") for c in cfgs]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=0)
    a.encode_traversal(6, stream=side)  # the weights move from the fourth pass
    for c, o in zip(cfgs, outs):
        a.degrees_enqueue(c, o.data_ptr(), stream=side)
    a.encode_traversal(2, stream=side)
    side.synchronize()  # the only synchronise
    twin.encode_traversal(6)
    syn = twin.download_synapses()
    for c, o, (neurons, what) in zip(cfgs, outs, ((None, 15), ((256, 256), ("in", "in_w")))):
        got = degree.decode(o.cpu().numpy().view(np.uint64), c, n_nrn)
        want = twin.degrees(neurons, what)
        _same(got, want)
        _same(want, degree.reference(syn, c, n_nrn))
    with make() as fresh:
        first = fresh.degrees((256, 256), ("in", "in_w"))
    assert not np.array_equal(_words(first), _words(want))  # the passes before the census moved the weights
    twin.encode_traversal(2)
    assert a.checksum() == twin.checksum()  # the census wrote nothing but its result
    assert np.array_equal(a.last_fired(), twin.last_fired()) and a.scalars() == twin.scalars()
    bad = degree.config((5, 0), 15)
    with pytest.raises(abnn_amd.AbnnError) as err:
        a.degrees_enqueue(bad, outs[0].data_ptr())
    assert err.value.status == 1
    a.close()
    twin.close()


# ---- 8. shards ---------------------------------------------------------------------------------------------
def test_merge_of_three_shards_equals_the_unsharded_census(gpu):
    import abnn_amd
    from abnn_amd import degree
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
        for neurons, what in ((None, 15), ((256, 256), ("in", "in_w")), ((0, 20), 5), ((38, 2), 15)):
            parts = [s.degrees(neurons, what) for s in shards]
            assert [p["records"] for p in parts] == [3334, 3333, 3333]
            _same(degree.merge(parts), _against_reference(whole, neurons, what, syn=syn), str((neurons, what)))
        for s in shards:
            s.close()


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_sharded_brain_degrees_world1(gpu, monkeypatch):
    import torch.distributed as dist

    from abnn_amd.shard import ShardedBrain, TorchComm

    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(_port()))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        sb = ShardedBrain(TorchComm(), 256, 256, 488, 10_000, 100_000, device=0, native=True)
        sb.brain.build_random_graph(1)
        for neurons, what in ((None, 15), ((256, 256), ("in", "in_w")), ((0, 30), ("out",))):
            _same(sb.degrees(neurons, what), _against_reference(sb.brain, neurons, what), str((neurons, what)))
        sb.native.close()
        sb.brain.close()
    finally:
        dist.destroy_process_group()


# ---- 9. the C++ mirrors ----------------------------------------------------------------------------------------
def test_cpp_degrees(gpu):
    from abnn_amd.build import build_degree_test

    prog = build_degree_test()
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    lines = r.stdout.strip().splitlines()
    assert lines, (r.returncode, r.stderr[-2000:])
    res = json.loads(lines[-1])
    assert r.returncode == 0 and res["ok"], (res, r.stderr[-2000:])
    assert res["records"] == 100_000 == res["out_total"] and res["neurons"] == 10_000
    assert res["in_degree_of_outputs"] == 256
