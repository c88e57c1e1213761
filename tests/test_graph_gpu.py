"""The graph builder on the GPU (abnn.h abnn_build_graph, csrc/graph.hip).

Every comparison is Brain.build_graph followed by download_synapses() against
graph.reference (the rule in numpy), all 32-bit words equal: record counts
around the four-record quad, block boundaries at every residue mod 4, few
workgroups that loop, neuron ids whose src code uses its high bits, capacity
headroom, a built brain against an uploaded one through passes in both modes
and through structural updates, shards with odd offsets, refusals that leave
the records in place, and the degree census of a built ring."""
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
NONE = 0xFFFFFFFF


def _same(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = got.view(np.uint32).reshape(-1, 4), want.view(np.uint32).reshape(-1, 4)
    bad = np.flatnonzero((g != w).any(axis=1))
    assert bad.size == 0, (what, bad.size, bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist())


def _mixed_blocks(n_nrn=1000):
    """All three topologies and both laws; 259 records in front of the last
    block, the boundaries at 129, 130, 135, 259: 1, 2, 3, 3 mod 4."""
    from abnn_amd import graph

    return [
        graph.dense((0, 16), (16, 8), graph.uniform(0.4, 0.8), count=129),
        graph.random((24, 100), (30, 7), 1, graph.beta(2, 8)),                       # a one-record block
        graph.small_world((100, 9), 8, 0.0, graph.beta(9, 3, -1.0, 1.0), count=5),   # a block of 5 records
        graph.small_world((50, n_nrn - 50), 4, 0.25, graph.beta(2, 8, 0.0, 0.5), count=124),
    ]


def _mixed_spec(total, n_nrn=1000, seed=0xABCDEF0123456789):
    """`total` records: the mixed blocks, cut where total is small, then random
    and ring blocks that share what is left."""
    from abnn_amd import graph

    blocks, left = [], total
    for b in _mixed_blocks(n_nrn):
        if left == 0:
            break
        b.count = min(b.count, left)
        blocks.append(b)
        left -= b.count
    if left:
        half = left // 2 + 1
        blocks.append(graph.random((24, n_nrn - 24), (0, n_nrn), half, graph.uniform(0.1, 0.2)))
        if left - half:
            blocks.append(graph.small_world((24, n_nrn - 24), 10, 0.1, graph.beta(2, 8), count=left - half))
    return graph.spec(blocks, seed)


def _brain(n_syn, **kw):
    import abnn_amd

    return abnn_amd.Brain(256, 256, 488, n_syn, 100_000, **kw)


# ---- 1. built equals the rule -----------------------------------------------------------------------------
@pytest.mark.parametrize("n_syn", [0, 1, 3, 4, 5, 129, 131, 255, 256, 257, 2_049, 70_003])
def test_build_equals_reference(gpu, n_syn):
    from abnn_amd import graph

    spec = _mixed_spec(max(n_syn, 1))
    assert graph.records(spec) == max(n_syn, 1)
    with _brain(n_syn) as b:
        b.build_graph(spec)
        _same(b.download_synapses(), graph.reference(spec, 0, n_syn), f"n_syn {n_syn}")
        # again over records that already hold something else: every record is rewritten
        if n_syn:
            b.build_random_graph(3)
            other = _mixed_spec(n_syn, seed=5)
            b.build_graph(other)
            _same(b.download_synapses(), graph.reference(other), f"n_syn {n_syn}, rebuilt")


def test_three_workgroups_loop_over_three_million_records(gpu, monkeypatch):
    import abnn_amd
    from abnn_amd import graph

    monkeypatch.setenv("ABNN_GRAPH_BLOCKS", "3")  # read at create: 3 workgroups, ~980 iterations each
    n_syn, n_nrn = 3_000_003, 100_512
    spec = _mixed_spec(n_syn, n_nrn)
    want = graph.reference(spec)
    for mode in (abnn_amd._lib.MODE_SWEEP, abnn_amd._lib.MODE_RANDOM):  # random mode: the src32 mirror is written too
        with abnn_amd.Brain(256, 256, 100_000, n_syn, 100_000, mode=mode) as b:
            b.build_graph(spec)
            _same(b.download_synapses(), want, f"mode {mode}")


# ---- 2. the src code's high bits ----------------------------------------------------------------------------
def test_neuron_ids_above_2_pow_23(gpu):
    import abnn_amd
    from abnn_amd import graph

    n_nrn = (1 << 24) - 2  # the largest N_NRN (below 2^24 - 1)
    top = n_nrn - 1
    u = graph.uniform(0.1, 0.2)
    spec = graph.spec([
        graph.dense(((1 << 23) - 5, 10), ((1 << 18) - 3, 7), u, count=141),           # src straddles 2^23, dst 2^18
        graph.random(((1 << 23) - 50_000, 100_000), (top - 9, 10), 20_001, graph.beta(2, 8)),
        graph.small_world(((1 << 23) - 1000, 2000), 6, 0.2, u, count=12_001),
        graph.random((0, n_nrn), (0, n_nrn), 30_000, u),                              # every bit of the code
        graph.small_world((top - 999, 1000), 3, 0.0, graph.beta(8, 8), count=3_002),  # the last neuron
    ], 17)
    n_syn = graph.records(spec)
    want = graph.reference(spec)
    assert want["src"].max() == top and want["src"].min() < 1 << 18 and n_syn % 4 != 0
    for mode in (abnn_amd._lib.MODE_SWEEP, abnn_amd._lib.MODE_RANDOM):
        with abnn_amd.Brain(256, 256, n_nrn - 512, n_syn, 4096, mode=mode) as b:
            b.build_graph(spec)
            _same(b.download_synapses(), want, f"mode {mode}")


# ---- 3. / 4. built equals uploaded, in behaviour ---------------------------------------------------------------
N_HID = 99_488
N_RUN = 1_000_003


def _run_spec():
    """The recipe's two blocks (dense input -> output, random hidden) and a
    small-world block over the hidden neurons with Beta(2, 8) weights."""
    from abnn_amd import graph

    r = graph.recipe(256, 256, N_HID, 800_003, seed=21)
    ring = graph.small_world((512, N_HID), 2, 0.1, graph.beta(2, 8, 0.05, 0.55), count=N_RUN - 800_003)
    return graph.spec([r.blocks[0], r.blocks[1], ring], 21)


@pytest.fixture(scope="module")
def run_reference():
    from abnn_amd import graph

    return graph.reference(_run_spec())


def _state(b):
    return {"n_syn": b.n_syn(), "checksum": b.checksum(), "last_fired": b.last_fired(), "scalars": b.scalars(),
            "stats": b.stats(), "census": b.census(64, 0.0, 1.0), "updates": b.structural_updates()}


def _assert_same_state(a, b, what):
    for k in a:
        if k == "last_fired":
            assert np.array_equal(a[k], b[k]), (what, k)
        elif k == "census":
            assert all(np.array_equal(a[k][f], b[k][f]) for f in a[k]), (what, k)
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


@pytest.mark.parametrize("case", ["sweep", "random", "structural"])
def test_built_brain_behaves_as_an_uploaded_one(gpu, run_reference, case):
    """Brain A is built on the device, brain B holds the same records by
    upload; both have headroom after n_syn (syn_capacity), so a store past
    n_syn would show in the padding that the sweep's last iteration reads.
    Eight passes over every record must leave the two in the same state."""
    import abnn_amd

    spec = _run_spec()
    kw = dict(syn_capacity=N_RUN + 4_099)
    if case == "random":
        kw["mode"] = abnn_amd._lib.MODE_RANDOM  # picks read the src32 mirror
    if case == "structural":
        kw.update(w_prune=0.15, compact_every=2)  # the tally of tombstones must be right after the build
    brains = [abnn_amd.Brain(256, 256, N_HID, N_RUN, N_RUN, **kw) for _ in range(2)]
    try:
        a, b = brains
        if case == "structural":  # A held tombstones before the build: their tally must not survive it
            old = run_reference.copy()
            old["src"][::7] = NONE
            old["dst"][::7] = NONE
            a.upload_synapses(old)
        a.build_graph(spec)
        b.upload_synapses(run_reference)
        _same(a.download_synapses(), run_reference, case)
        _assert_same_state(_state(a), _state(b), f"{case}: before the passes")
        for x in brains:
            x.set_auto_stimulus(0, 256)
            x.encode_traversal(8)
        sa, sb = _state(a), _state(b)
        _assert_same_state(sa, sb, f"{case}: after 8 passes")
        assert sa["stats"]["fired"] > 0 and sa["scalars"]["clock"] == 8
        _same(a.download_synapses(), b.download_synapses(), f"{case}: records after 8 passes")
        if case == "structural":
            assert sa["updates"] == 4
    finally:
        for x in brains:
            x.close()


# ---- 5. shards ---------------------------------------------------------------------------------------------
def test_three_shards_concatenate_to_the_unsharded_graph(gpu):
    import abnn_amd
    from abnn_amd import graph
    from abnn_amd.shard import global_events, shard_ranges

    n_syn, events = 10_003, 100_000
    spec = _mixed_spec(n_syn)
    want = graph.reference(spec)
    ranges = shard_ranges(n_syn, 3)
    assert [lo for lo, _ in ranges] == [0, 3335, 6669]  # odd offsets: 3 and 1 mod 4
    ge = global_events(n_syn, events, 3)
    parts = []
    for lo, hi in ranges:
        with abnn_amd.Brain(256, 256, 488, hi - lo, events, syn_offset=lo, global_events=ge) as s:
            s.build_graph(spec)
            parts.append(s.download_synapses())
    _same(np.concatenate(parts), want, "three shards")
    # slices that cut the small blocks mid-quad, from every offset residue
    for lo, n in ((1, 130), (127, 9), (129, 1), (130, 6), (131, 257), (258, 1031)):
        with abnn_amd.Brain(256, 256, 488, n, events, syn_offset=lo, global_events=ge) as s:
            s.build_graph(spec)
            _same(s.download_synapses(), want[lo:lo + n], f"slice {lo} + {n}")
    # a shard far into a graph: record indices above 2^32 within a block
    far = graph.spec([graph.dense((0, 700), (100, 900), graph.uniform(0.0, 1.0), count=1 << 34),
                      graph.small_world((0, 1000), 7, 0.5, graph.beta(2, 8), count=1 << 34)], 3)
    for lo in ((1 << 32) - 1001, (1 << 34) - 1003, (1 << 34) + (1 << 33) + 1):
        with abnn_amd.Brain(256, 256, 488, 2_003, events, syn_offset=lo, global_events=ge) as s:
            s.build_graph(far)
            _same(s.download_synapses(), graph.reference(far, lo, 2_003), f"far {lo}")


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_sharded_brain_build_graph_world1(gpu, monkeypatch):
    import torch.distributed as dist

    from abnn_amd import graph
    from abnn_amd.shard import ShardedBrain, TorchComm

    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(_port()))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        sb = ShardedBrain(TorchComm(), 256, 256, 488, 10_001, 100_000, device=0)
        spec = _mixed_spec(10_001)
        sb.build_graph(spec)
        _same(sb.brain.download_synapses(), graph.reference(spec), "world 1")
        for total in (10_000, 10_002):  # a spec of another size than the sharded graph
            with pytest.raises(ValueError):
                sb.build_graph(_mixed_spec(total))
        bad = _mixed_spec(10_001)
        bad.reserved = 1
        with pytest.raises(ValueError):
            sb.build_graph(bad)
        _same(sb.brain.download_synapses(), graph.reference(spec), "world 1, after the refusals")
        sb.brain.close()
    finally:
        dist.destroy_process_group()


# ---- 6. refusals on a live handle ------------------------------------------------------------------------------
def test_refusals_leave_the_records_in_place(gpu):
    import abnn_amd
    from abnn_amd import graph

    n_syn = 5_001
    spec = _mixed_spec(n_syn)
    want = graph.reference(spec)
    u = graph.uniform(0.0, 1.0)
    with _brain(n_syn) as b:  # N_NRN = 1000
        b.build_graph(spec)
        invalid = _mixed_spec(n_syn)
        invalid.blocks[0].reserved[0] = 1
        refused = {
            "src population ends above N_NRN": graph.spec([graph.random((0, 1001), (0, 10), n_syn, u)], 1),
            "dst population ends above N_NRN": graph.spec([graph.random((0, 10), (999, 2), n_syn, u)], 1),
            "ring population ends above N_NRN": graph.spec([graph.small_world((500, 501), 3, 0.0, u, count=n_syn)], 1),
            "a later block's population": graph.spec([graph.random((0, 10), (0, 10), n_syn - 1, u),
                                                      graph.dense((1000, 1), (0, 1), u)], 1),
            "fewer records than n_syn": _mixed_spec(n_syn - 1),
            "an invalid spec": invalid,
        }
        for name, s in refused.items():
            with pytest.raises(abnn_amd.AbnnError) as err:
                b.build_graph(s)
            assert err.value.status == 1, name
            _same(b.download_synapses(), want, name)
        b.build_graph(_mixed_spec(n_syn + 1))  # a longer spec is fine: the handle takes its first n_syn records
        _same(b.download_synapses(), graph.reference(_mixed_spec(n_syn + 1), 0, n_syn), "a longer spec")
    with abnn_amd.Brain(256, 256, 488, 100, 1000, syn_offset=4_902) as s:  # 4902 + 100 > 5001
        s.build_random_graph(1)
        before = s.download_synapses()
        with pytest.raises(abnn_amd.AbnnError) as err:
            s.build_graph(spec)
        assert err.value.status == 1
        _same(s.download_synapses(), before, "syn_offset + n_syn above the total")


# ---- 7. the degree census of a built ring -------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 5, 299])
def test_degrees_of_a_built_ring(gpu, k):
    from abnn_amd import graph

    first, n = 700, 300
    spec = graph.spec([graph.small_world((first, n), k, 0.0, graph.uniform(0.2, 0.4))], 8)
    with _brain(n * k) as b:
        b.build_graph(spec)
        d = b.degrees((first, n), ("out", "in"))
        assert d["out"].tolist() == [k] * n and d["in"].tolist() == [k] * n
        every = b.degrees(None, ("out", "in"))
        assert int(every["out"].sum()) == n * k == int(every["in"][first:].sum())
