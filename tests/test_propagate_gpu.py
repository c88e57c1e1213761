"""Signal propagation on the GPU (abnn.h abnn_propagate_*, csrc/propagate.hip).

Every comparison is the device's words against abnn_propagate_host (the same
rule on the host, csrc/propagate.h) over the same brain's download_synapses(),
all result words equal: record-count edges of every instantiation, the sparse,
the dense and the chosen forward path, narrow and wide out-ranges, runs of
equal keys, sums that wrap 2**64, tombstones and capacity headroom, neuron ids
up to the last valid one, another base_scale, the iteration and its rescale,
the enqueue-only path between passes, shards and the C++ mirrors."""
import json
import socket
import subprocess

import numpy as np
import pytest

from propagate_helpers import NONE, one_hot, plane, records

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = float("inf")
AUTO, SPARSE, DENSE = 0, 1, 2


def _brain(n_syn, n_hidden=488, **kw):
    import abnn_amd

    return abnn_amd.Brain(256, 256, n_hidden, n_syn, 100_000, **kw)


def _set_path(b, path):
    from abnn_amd import _lib

    _lib.call("abnn_debug_set_propagate_path", b._h, path)


def _device(b, x, **kw):
    from abnn_amd import propagate as P

    return P.to_words(b.propagate(x, **kw))


def _check(b, syn, x, note="", paths=(SPARSE, DENSE, AUTO), **kw):
    """The device's words on every forward path against the host rule; returns the decoded result."""
    from abnn_amd import propagate as P

    cfg = P.config(**kw)
    n_nrn = b.n_neuron()
    want = P.host(syn, cfg, n_nrn, x, b.params.base_scale)
    for path in (paths if not kw.get("reverse") else (AUTO,)):  # the transpose has one instance
        _set_path(b, path)
        got = _device(b, x, **kw)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (note, kw, path, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
    _set_path(b, AUTO)
    return P.decode(want, cfg, n_nrn)


def _sparse_x(n_nrn, seed):
    """About one neuron in 64 non-zero: the device chooses the sparse path."""
    x = plane(n_nrn, seed, 0.0)
    x[np.random.default_rng(seed).random(n_nrn) >= 1 / 64] = 0
    return x


# ---- 1. record-count edges -------------------------------------------------------------------------
# a sparse iteration of one workgroup is 8192 records (8 x 512 threads x 2 loads), a dense or transposed
# one 4096 (2 x 512 x 4); n % 8 records are in no whole sparse load, an odd n's last one in no pair
@pytest.mark.parametrize("n_syn", [0, 1, 7, 8, 9, 127, 128, 129, 4095, 4096, 4097, 8191, 8192, 8193, 100_003])
def test_record_count_edges(gpu, n_syn):
    n_nrn = 1000
    with _brain(n_syn) as b:
        syn = records(n_syn, n_syn + 1, n_nrn)
        if 0 < n_syn < 300:  # few records: let the last ones meet a non-zero x
            syn["src"][-3:] = [5, 999, 5][-min(3, n_syn):]
            syn["dst"][-3:] = [999, 5, 6][-min(3, n_syn):]
        if n_syn:
            b.upload_synapses(syn)
        back = b.download_synapses() if n_syn else syn
        assert np.array_equal(back.view(np.uint32), syn.view(np.uint32))
        full, thin = plane(n_nrn, 3, 0.2), _sparse_x(n_nrn, 4)
        full[[5, 999]] = [1 << 30, -7]
        thin[[5, 999]] = [-(1 << 31), 3]
        for reverse in (False, True):
            for x in (full, thin):
                d = _check(b, back, x, f"n {n_syn}", reverse=reverse)
                assert d["records"] == n_syn and d["tombstones"] == int((back["dst"] == NONE).sum())
            _check(b, back, full, f"n {n_syn}", reverse=reverse, fire_p=True, weights=(-0.5, 0.75), outputs=(0, 999))
        if n_syn == 100_003:
            assert d["followed"] > 500 and d["skipped"] > 0


# ---- 2. out-ranges, in-ranges, densities ------------------------------------------------------------
@pytest.fixture(scope="module")
def mid():
    """One brain of 60 001 records over 6 512 neurons, uploaded once; the tests below only read it."""
    syn = records(60_001, 17, 6512)
    syn.setflags(write=False)
    b = _brain(60_001, n_hidden=6000)
    b.upload_synapses(syn)
    yield b, syn
    b.close()


@pytest.mark.parametrize("outputs", [(4000, 1), (100, 4096), (100, 4097), None])
def test_out_ranges_narrow_and_wide(gpu, mid, outputs):
    from abnn_amd import propagate as P

    b, syn = mid
    n_nrn = b.n_neuron()
    assert n_nrn == 6512 and P.NARROW_MAX == 4096
    hot = one_hot(n_nrn, int(syn["src"][syn["dst"] == 4000][0]) if outputs == (4000, 1) else 300)
    for x in (hot, _sparse_x(n_nrn, 5), plane(n_nrn, 6, 0.0)):
        for reverse in (False, True):
            _check(b, syn, x, reverse=reverse, outputs=outputs)
        _check(b, syn, x, inputs=(512, 3000), outputs=outputs, fire_p=True)      # part of the graph is outside
        _check(b, syn, x, inputs=(3000, 3512), outputs=outputs, reverse=True, weights=(0.0, INF))
    x = plane(n_nrn, 6, 0.0)
    d = _check(b, syn, x, outputs=outputs)
    assert d["followed"] > 0 and d["nnz"] == int(np.count_nonzero(x)) > n_nrn // 2


def test_the_device_chooses_by_the_nonzero_count(gpu, mid):
    """The choice is not observable in the words: both sides of the crossover give the host's."""
    from abnn_amd import propagate as P

    b, syn = mid
    n_nrn = b.n_neuron()
    edge = n_nrn // P.SPARSE_DIV
    for nnz in (0, 1, edge - 1, edge, edge + 1, edge + 2, n_nrn):
        x = np.zeros(n_nrn, dtype=np.int32)
        x[np.random.default_rng(nnz).choice(n_nrn, nnz, replace=False)] = 12345
        d = _check(b, syn, x, f"nnz {nnz}", paths=(AUTO,))
        assert d["nnz"] == nnz and d["sum_abs_x"] == 12345 * nnz
        assert d["followed"] == 0 if nnz == 0 else d["followed"] > 0 or nnz == 1


# ---- 3. runs --------------------------------------------------------------------------------------------
def test_every_record_on_one_pair(gpu):
    from abnn_amd import SYN_DTYPE

    n = 10_001
    syn = np.zeros(n, dtype=SYN_DTYPE)
    syn["src"], syn["dst"], syn["w"] = 5, 9, 0.3
    syn["w"][::7] = -0.9
    syn["w"][3::1000] = np.nan
    with _brain(n) as b:
        b.upload_synapses(syn)
        x = plane(1000, 8, 0.0)
        x[[5, 9]] = [-123_456_789, 1 << 30]
        for reverse in (False, True):
            for outputs in (None, (0, 16)):
                d = _check(b, syn, x, reverse=reverse, outputs=outputs)
                assert d["followed"] == n and d["skipped"] == len(syn["w"][3::1000])
                assert np.count_nonzero(d["y"]) == 1


def test_sorted_by_dst_and_the_dense_block(gpu):
    with _brain(100_000) as b:
        b.build_random_graph(1)
        before = b.download_synapses()
        x = plane(1000, 9, 0.1)
        block = _check(b, before, x, inputs=(0, 256), outputs=(256, 256))  # the dense input -> output block: 256 records per src
        assert block["followed"] >= int((x[:256] != 0).sum()) * 256
        back = _check(b, before, x, inputs=(256, 256), outputs=(0, 256), reverse=True)  # its transpose: 256 records per kout
        assert back["followed"] >= int((x[256:512] != 0).sum()) * 256
        _check(b, before, x, reverse=True)  # runs of equal src through the wide path
        b.reorder("dst")
        syn = b.download_synapses()
        assert (np.diff(syn["dst"].astype(np.int64)) >= 0).all() and not np.array_equal(syn, before)
        for outputs in (None, (256, 256)):
            _check(b, syn, x, outputs=outputs, fire_p=True)
        whole = _check(b, syn, x)
        assert np.array_equal(whole["y"], _check(b, before, x, paths=())["y"])  # the host's y of the old order: the order does not matter


# ---- 4. sums modulo 2**64 ---------------------------------------------------------------------------------
def test_sums_wrap_identically_on_host_and_device(gpu):
    from abnn_amd import SYN_DTYPE

    n_a, n_b = 1 << 19, (1 << 19) + (1 << 13)
    syn = np.zeros(n_a + n_b, dtype=SYN_DTYPE)
    syn["src"], syn["w"] = 7, 127.5
    syn["dst"][:n_a], syn["dst"][n_a:] = 400, 401
    q = int(127.5 * (1 << 24))
    term = (q << 30) >> 16
    assert n_a * term > 1 << 63 and n_b * term > 1 << 64  # past the sign bit, and past the word
    with _brain(n_a + n_b) as b:
        b.upload_synapses(syn)
        x = one_hot(1000, 7)
        for outputs in (None, (400, 2)):
            d = _check(b, syn, x, outputs=outputs)
            y = d["y"].view(np.uint64)[[400, 401] if outputs is None else [0, 1]]
            assert [int(v) for v in y] == [n_a * term % (1 << 64), n_b * term % (1 << 64)]
        x = np.zeros(1000, dtype=np.int32)
        x[[400, 401]] = 1 << 30
        d = _check(b, syn, x, reverse=True)
        assert int(d["y"].view(np.uint64)[7]) == (n_a + n_b) * term % (1 << 64)


# ---- 5. tombstones and headroom ---------------------------------------------------------------------------
def test_tombstones_after_a_lesion_and_capacity_headroom(gpu):
    syn = records(5_003, 3, 1000, dead=0.0)
    with _brain(5_003, syn_capacity=9_000) as b:  # the capacity beyond n_syn is never read
        b.upload_synapses(syn)
        killed = b.edit("kill", src=(100, 300))["killed"]
        back = b.download_synapses()
        assert killed > 500 and int((back["dst"] == NONE).sum()) == killed
        x = plane(1000, 11, 0.3)
        for reverse in (False, True):
            d = _check(b, back, x, reverse=reverse)
            assert d["records"] == 5_003 and d["tombstones"] == killed
            _check(b, back, x, reverse=reverse, outputs=(50, 500), weights=(-0.25, 0.9))


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
    x = plane(b.n_neuron(), 12, 0.5)
    before = _check(b, syn, x, fire_p=True)
    assert before["tombstones"] == 20_000
    b.set_auto_stimulus(0, 256)
    b.encode_traversal(2)  # the second pass runs the structural update: the tombstones are removed
    assert b.n_syn() <= n_syn - 20_000
    after_syn = b.download_synapses()
    for reverse in (False, True):
        after = _check(b, after_syn, x, fire_p=True, reverse=reverse)
        assert after["records"] == b.n_syn() < before["records"] and after["tombstones"] == 0
    b.close()


# ---- 6. high neuron ids --------------------------------------------------------------------------------------
def test_high_neuron_ids(gpu):
    import abnn_amd
    import high_id_helpers as H

    n_nrn = 2 ** 24 - 2  # the largest N_NRN: src codes of every class, the map's last word is partial
    parts = H.high_id_parts(n_nrn)
    syn = parts["syn"]
    ids = np.unique(np.concatenate([H.fixed_ids(n_nrn), parts["probes"], [n_nrn - 1, n_nrn - 2, (1 << 18) + 1]]))
    assert ids.max() == n_nrn - 1 and (ids > 1 << 18).sum() > 100
    x = np.zeros(n_nrn, dtype=np.int32)
    x[ids] = np.random.default_rng(2).integers(1, 1 << 30, len(ids))
    with abnn_amd.Brain(256, 256, n_nrn - 512, len(syn), 100_000) as b:
        assert b.n_neuron() == n_nrn
        b.upload_synapses(syn)
        fwd = _check(b, syn, x, paths=(SPARSE, DENSE))  # the probes' own records leave them
        assert fwd["followed"] >= len(parts["probes"])
        rev = _check(b, syn, x, reverse=True)           # ... and the crafted first-layer records enter them
        assert rev["followed"] >= len(parts["probes"])
        _check(b, syn, x, paths=(AUTO,), inputs=(1 << 18, n_nrn - (1 << 18)), outputs=(n_nrn - 4097, 4097))
        _check(b, syn, x, reverse=True, inputs=(n_nrn - 4096, 4096), outputs=(0, 256), fire_p=True)
        # more non-zero x than the LDS fold of the map takes, over a map that does not fit it
        from abnn_amd import propagate as P

        many = np.zeros(n_nrn, dtype=np.int32)
        many[n_nrn - 70_000:] = 3
        assert 70_000 > P.FOLD_MAX_NNZ and n_nrn > 32 * P.FOLD_WORDS
        assert 70_000 * P.SPARSE_DIV < n_nrn  # the device still chooses the sparse path
        _check(b, syn, many, paths=(AUTO,), outputs=(256, 4096))


# ---- 7. another base_scale -------------------------------------------------------------------------------------
def test_fire_p_takes_the_handles_base_scale(gpu):
    from abnn_amd import propagate as P

    syn = records(20_000, 21, 1000)
    x = plane(1000, 22, 0.2)
    with _brain(20_000, base_scale=0.37) as b:
        assert b.params.base_scale == F32(0.37)
        b.upload_synapses(syn)
        d = _check(b, syn, x, fire_p=True)
        other = P.decode(P.host(syn, P.config(fire_p=True), 1000, x, 0.8), P.config(fire_p=True), 1000)
        assert d["followed"] == other["followed"] and not np.array_equal(d["y"], other["y"])
        _check(b, syn, x, fire_p=True, reverse=True, outputs=(3, 700))


# ---- 8. iterate ----------------------------------------------------------------------------------------------------
def _host_iterate(syn, cfg, n_nrn, x, steps, base_scale):
    from abnn_amd import propagate as P

    trace = np.zeros((steps, 8), dtype=np.uint64)
    for k in range(steps):
        x, trace[k] = P.rescale_host(P.host(syn, cfg, n_nrn, x, base_scale), cfg, n_nrn, x)
    return x, trace


def test_iterate_equals_the_host_rule_row_by_row(gpu):
    import torch

    from abnn_amd import propagate as P

    n_nrn, steps = 1000, 6
    syn = records(30_000, 31, n_nrn)
    syn["w"] = np.abs(syn["w"])  # NaN, inf and 200 stay: skipped records in every row
    with _brain(30_000) as b:
        b.upload_synapses(syn)
        for neurons, reverse, fire_p in ((None, False, True), ((256, 700), True, False), ((10, 980), False, False)):
            cfg = P.config(neurons, neurons, reverse, fire_p)
            x0 = np.zeros(n_nrn, dtype=np.int32)
            first, count = P.ranges(cfg, n_nrn)[:2]
            x0[first:first + count] = P.ONE >> 1
            x0[5] = -77  # outside the third range: never touched
            want_x, want_trace = _host_iterate(syn, cfg, n_nrn, x0, steps, b.params.base_scale)
            got = b.branching(steps, neurons, fire_p, reverse, x0=x0)
            assert np.array_equal(got["x"], want_x)
            want = P.branching(want_trace)
            for k in ("nnz", "sum_abs_x", "sum_abs_y", "max_abs_y", "e", "followed", "skipped", "estimates"):
                assert np.array_equal(got[k], want[k]), k
            assert got["ratio"] > 0 and (got["skipped"] > 0).all()
            # six separate propagate + rescale enqueues
            x = torch.from_numpy(x0).to("cuda:0")
            out = torch.zeros(P.n_words(cfg, n_nrn), dtype=torch.int64, device="cuda:0")
            trace = torch.zeros(steps * 8, dtype=torch.int64, device="cuda:0")
            for k in range(steps):
                b.propagate_enqueue(cfg, x.data_ptr(), out.data_ptr())
                b.propagate_rescale_enqueue(cfg, out.data_ptr(), x.data_ptr(), trace.data_ptr() + 64 * k)
            torch.cuda.synchronize()
            assert np.array_equal(x.cpu().numpy(), want_x)
            assert np.array_equal(trace.cpu().numpy().view(np.uint64).reshape(steps, 8), want_trace)
        # the default start, the numpy restatement
        got = b.branching(4)
        _, want_trace = P.iterate_reference(syn, P.config(fire_p=True), n_nrn, np.full(n_nrn, P.ONE >> 1, dtype=np.int32), 4,
                                            b.params.base_scale)
        assert np.array_equal(got["estimates"], P.branching(want_trace)["estimates"])


def test_iterate_on_a_graph_that_dies_out(gpu):
    import abnn_amd
    from abnn_amd import SYN_DTYPE
    from abnn_amd import propagate as P

    syn = np.zeros(3, dtype=SYN_DTYPE)  # a chain of three records: 10 -> 11 -> 12 -> 13
    syn["src"], syn["dst"], syn["w"] = [10, 11, 12], [11, 12, 13], 0.5
    with _brain(3) as b:
        b.upload_synapses(syn)
        x0 = one_hot(1000, 10)
        got = b.branching(6, fire_p=False, x0=x0)
        want_x, want_trace = _host_iterate(syn, P.config(), 1000, x0, 6, 0.0)
        assert np.array_equal(got["x"], want_x) and not got["x"].any()
        assert got["followed"].tolist() == [1, 1, 1, 0, 0, 0] and got["estimates"].tolist() == [0.5, 0.5, 0.5, 0, 0, 0]
        assert got["nnz"].tolist() == [1, 1, 1, 1, 0, 0] and got["e"].tolist()[3:] == [0, 0, 0]
        assert not want_trace[3, 2:].any() and not want_trace[4:].any()  # y is zero from the fourth step, x from the fifth
        for k in ("sum_abs_x", "sum_abs_y", "max_abs_y", "skipped"):
            assert np.array_equal(got[k], P.branching(want_trace)[k]), k
        # refused on the host, before any launch
        import torch

        t = torch.zeros(2048, dtype=torch.int64, device="cuda:0")
        for bad, steps in ((P.config((0, 10), (0, 11)), 2), (P.config(), 0), (P.config(), P.PROP_MAX_STEPS + 1),
                           (P.config(weights=(1.0, 0.5)), 2)):
            with pytest.raises(abnn_amd.AbnnError) as err:
                b.propagate_iterate_enqueue(bad, steps, t.data_ptr(), t.data_ptr(), t.data_ptr())
            assert err.value.status == 1
        with pytest.raises(abnn_amd.AbnnError) as err:
            b.propagate_enqueue(P.config(), t.data_ptr() + 4, t.data_ptr())  # x is not 16-byte aligned
        assert err.value.status == 1


# ---- 9. between passes -------------------------------------------------------------------------------------------
def test_enqueue_between_passes_on_a_side_stream(gpu):
    import torch

    import abnn_amd
    from abnn_amd import propagate as P

    def make():
        b = abnn_amd.Brain(256, 256, 99_488, 1_000_000, 1_000_000)
        b.build_random_graph(1)
        b.set_auto_stimulus(0, 256)
        return b

    a, twin = make(), make()
    n_nrn = a.n_neuron()
    x0 = plane(n_nrn, 41, 0.5)
    cfgs = [P.config(fire_p=True), P.config(reverse=True, outputs=(0, 256)), P.config(fire_p=True)]
    outs = [torch.zeros(P.n_words(c, n_nrn), dtype=torch.int64, device="cuda:0") for c in cfgs]
    x = torch.from_numpy(x0).to("cuda:0")
    hid = P.config((512, n_nrn - 512), (512, n_nrn - 512), fire_p=True)
    xi = torch.from_numpy(x0).to("cuda:0")
    work = torch.zeros(P.n_words(hid, n_nrn), dtype=torch.int64, device="cuda:0")
    trace = torch.zeros(3 * 8, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=0)
    a.encode_traversal(6, stream=side)  # the weights move from the fourth pass
    for c, o in zip(cfgs, outs):
        a.propagate_enqueue(c, x.data_ptr(), o.data_ptr(), stream=side)
    a.propagate_iterate_enqueue(hid, 3, xi.data_ptr(), work.data_ptr(), trace.data_ptr(), stream=side)
    a.encode_traversal(2, stream=side)
    side.synchronize()  # the only synchronise
    twin.encode_traversal(6)
    syn = twin.download_synapses()
    for c, o in zip(cfgs, outs):
        assert np.array_equal(o.cpu().numpy().view(np.uint64), P.host(syn, c, n_nrn, x0, a.params.base_scale))
    assert torch.equal(outs[0], outs[2])
    want_x, want_trace = _host_iterate(syn, hid, n_nrn, x0, 3, a.params.base_scale)
    assert np.array_equal(xi.cpu().numpy(), want_x)
    assert np.array_equal(trace.cpu().numpy().view(np.uint64).reshape(3, 8), want_trace)
    twin.encode_traversal(2)
    assert a.checksum() == twin.checksum()  # the propagation wrote nothing but its results
    assert np.array_equal(a.download_synapses().view(np.uint32), twin.download_synapses().view(np.uint32))
    assert np.array_equal(a.last_fired(), twin.last_fired()) and a.scalars() == twin.scalars()
    assert a.stats() == twin.stats()
    a.close()
    twin.close()


def test_between_two_engine_runs(gpu):
    import torch

    import abnn_amd
    from abnn_amd import propagate as P

    def make():
        b = abnn_amd.Brain(256, 256, 9_488, 200_000, 200_000)
        b.build_random_graph(1)
        return b, abnn_amd.LearnEngine(b)

    rng = np.random.default_rng(5)
    frames, expect = rng.random((8, 256), dtype=F32), rng.random((8, 256), dtype=F32)
    (a, ea), (twin, et) = make(), make()
    n_nrn = a.n_neuron()
    cfg = P.config(fire_p=True)
    x0 = np.full(n_nrn, P.ONE >> 1, dtype=np.int32)
    x = torch.from_numpy(x0).to("cuda:0")
    work = torch.zeros(P.n_words(cfg, n_nrn), dtype=torch.int64, device="cuda:0")
    trace = torch.zeros(4 * 8, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=0)
    ea.run(frames[:4], expect[:4], stream=side)
    a.propagate_iterate_enqueue(cfg, 4, x.data_ptr(), work.data_ptr(), trace.data_ptr(), stream=side)
    ea.run(frames[4:], expect[4:], stream=side)
    side.synchronize()
    et.run(frames[:4], expect[:4])
    twin.synchronize()
    syn = twin.download_synapses()
    _, want_trace = _host_iterate(syn, cfg, n_nrn, x0, 4, a.params.base_scale)
    got = trace.cpu().numpy().view(np.uint64).reshape(4, 8)
    assert np.array_equal(got, want_trace) and P.branching(got)["ratio"] > 0
    et.run(frames[4:], expect[4:])
    twin.synchronize()
    assert np.array_equal(a.download_synapses().view(np.uint32), twin.download_synapses().view(np.uint32))
    assert np.array_equal(a.last_fired(), twin.last_fired()) and a.scalars() == twin.scalars()
    assert a.stats() == twin.stats() and str(ea.state()) == str(et.state())
    for h in (ea, et, a, twin):
        h.close()


# ---- 10. shards, the C++ mirrors, device memory ----------------------------------------------------------------
def test_stepped_shards_merge_to_the_unsharded_result(gpu):
    import abnn_amd
    from abnn_amd import propagate as P
    from abnn_amd.shard import global_events, shard_ranges

    n_syn, events, n_nrn = 10_001, 100_000, 1000
    syn = records(n_syn, 7, n_nrn)
    syn["w"][::5] = 127.5
    x = plane(n_nrn, 8, 0.2)
    x[::9] = -(1 << 31)
    ge = global_events(n_syn, events, 3)
    with _brain(n_syn) as whole:
        whole.upload_synapses(syn)
        shards = []
        for lo, hi in shard_ranges(n_syn, 3):
            s = abnn_amd.Brain(256, 256, 488, hi - lo, events, syn_offset=lo, global_events=ge)
            s.upload_synapses(syn[lo:hi])
            shards.append(s)
        for kw in ({}, {"reverse": True, "outputs": (100, 300)}, {"fire_p": True, "weights": (-1.0, 1.0), "inputs": (0, 900)}):
            want = _check(whole, syn, x, **kw)
            merged = P.merge([s.propagate(x, **kw) for s in shards])
            assert np.array_equal(P.to_words(merged), P.to_words(want)), kw
        for s in shards:
            s.close()


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_sharded_brain_propagate_and_branching_world1(gpu, monkeypatch):
    import torch.distributed as dist

    from abnn_amd import propagate as P
    from abnn_amd.shard import ShardedBrain, TorchComm

    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(_port()))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        sb = ShardedBrain(TorchComm(), 256, 256, 488, 100_000, 100_000, device=0, native=True)  # past the dense block
        sb.brain.build_random_graph(1)
        syn = sb.brain.download_synapses()
        x = plane(1000, 9, 0.3)
        for kw in ({}, {"reverse": True, "fire_p": True}, {"inputs": (0, 256), "outputs": (256, 256)}):
            want = P.host(syn, P.config(**kw), 1000, x, sb.brain.params.base_scale)
            assert np.array_equal(P.to_words(sb.propagate(x, **kw)), want), kw
        got, alone = sb.branching(5, (512, 488)), sb.brain.branching(5, (512, 488))
        assert np.array_equal(got["x"], alone["x"]) and np.array_equal(got["estimates"], alone["estimates"])
        assert np.array_equal(got["followed"], alone["followed"]) and got["ratio"] == alone["ratio"] > 0
        sb.native.close()
        sb.brain.close()
    finally:
        dist.destroy_process_group()


def test_cpp_propagate(gpu):
    from abnn_amd.build import build_propagate_test

    prog = build_propagate_test()
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    lines = r.stdout.strip().splitlines()
    assert lines, (r.returncode, r.stderr[-2000:])
    res = json.loads(lines[-1])
    assert r.returncode == 0 and res["ok"], (res, r.stderr[-2000:])
    assert res["records"] == 100_000 and res["neurons"] == 10_000
    assert res["followed"] > 10_000 and res["outputs_followed"] == 256 and res["steps"] == 6 and res["ratio"] > 0


def test_device_memory_returns_to_its_baseline(gpu):
    import torch

    from abnn_amd import _lib
    from abnn_amd import propagate as P

    live = _lib.load().abnn_debug_live_allocations
    base = int(live())
    b = _brain(5_000)
    b.upload_synapses(records(5_000, 1, 1000))
    created = int(live())
    x = plane(1000, 2)
    b.propagate(x)                       # the map, the rescale's words, the staged x and the result
    after = int(live())
    assert after == created + 4
    b.propagate(x, outputs=(0, 10))      # a smaller result: nothing new
    b.branching(3)
    t = torch.from_numpy(x).to("cuda:0")
    out = torch.zeros(P.n_words(P.config(), 1000), dtype=torch.int64, device="cuda:0")
    b.propagate_enqueue(P.config(), t.data_ptr(), out.data_ptr())
    b.propagate_rescale_enqueue(P.config(), out.data_ptr(), t.data_ptr())
    torch.cuda.synchronize()
    assert int(live()) == after
    b.close()
    assert int(live()) == base
