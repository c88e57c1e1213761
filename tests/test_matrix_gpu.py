"""The population connectivity matrix on the GPU (abnn.h abnn_matrix_*, csrc/matrix.hip).

Every comparison is Brain.matrix against matrix.reference over the same brain's
download_synapses(), all result words equal (every plane is an integer: the
tolerance is zero), on each kernel path abnn_debug_set_matrix_path exposes:
record-count edges, cell patterns that exercise the wave-uniform add and the run
heads at lane and wave boundaries, label planes (packed and direct, with
none-values, ids that are no neuron, an odd N_NRN), composition with hops and
components results on one stream, neuron ids up to the last valid one,
tombstones and capacity headroom, a structural update, the enqueue-only path on
a side stream between passes, shards, the C++ mirrors and the device allocations."""
import ctypes as C
import json
import socket
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
NONE = 0xFFFFFFFF
# the special weights of tests/test_hops_gpu.py
SPECIAL = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-40, 127.99999, 128.0, -128.0, -127.99999, 0.001, 2.0 ** -24,
                    2.0 ** -25, -(2.0 ** -24)], dtype=F32)
ALL = ("count", "w", "p")
BOUNDS_PATHS = (0, 1, 3)      # auto, runs, atomics (the lookup half of the path is LABELS')
LABELS_PATHS = (0, 1, 2, 3, 4)  # auto, runs / atomics x packed / direct
N_NRN = 1000


def _set_path(b, path):
    from abnn_amd import _lib

    _lib.call("abnn_debug_set_matrix_path", b._h, path)


def _same(got, want, what=""):
    from abnn_amd import matrix

    g, w = matrix.to_words(got), matrix.to_words(want)
    assert g.shape == w.shape, what
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (what, bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist())


def _against_reference(b, bounds=None, labels=None, pops=None, what=ALL, weights=None, syn=None, paths=None, note=""):
    """Brain.matrix on every path against the reference; labels is a numpy plane (uploaded once)."""
    import torch

    from abnn_amd import matrix

    syn = b.download_synapses() if syn is None else syn
    n_nrn = b.n_neuron()
    if labels is None and bounds is None:
        bounds = matrix.io_bounds(b.n_input(), b.n_output(), b.n_hidden())
    n_pops = len(bounds) - 1 if labels is None else pops
    cfg = matrix.config(n_pops, what, labels is not None, weights)
    want = matrix.reference(syn, cfg, n_nrn, b.params.base_scale, bounds=bounds, labels=labels)
    dev = None if labels is None else torch.from_numpy(np.ascontiguousarray(labels, dtype=np.uint32).view(np.int32)).to("cuda:0")
    got = None
    for path in paths or (BOUNDS_PATHS if labels is None else LABELS_PATHS):
        _set_path(b, path)
        got = b.matrix(bounds, dev, pops, what, weights)
        _same(got, want, f"{note} path {path} pops {n_pops} what {what} weights {weights}")
    _set_path(b, 0)
    assert got["tombstones"] + got["counted"] + got["src_unassigned"] + got["dst_unassigned"] + got["unassigned"] \
        + got["out_of_band"] == got["records"] == len(syn)
    assert int(got["sizes"].sum()) == got["assigned"]
    if "count" in what:
        assert int(got["count"].sum()) == got["counted"]
    return got


def _syn(src, dst, w=0.5):
    from abnn_amd import SYN_DTYPE

    syn = np.zeros(len(src), dtype=SYN_DTYPE)
    syn["src"], syn["dst"], syn["w"] = src, dst, w
    return syn


def _weights(n, seed):
    """Weights in [-0.1, 1.1] with the special values at the first, a middle and the last index."""
    w = np.random.default_rng(seed).uniform(-0.1, 1.1, n).astype(F32)
    k = len(SPECIAL)
    if n >= 3 * k:
        for at in (0, n // 2 - k // 2, n - k):
            w[at:at + k] = SPECIAL
    else:
        for j, at in enumerate(sorted({0, n // 2, n - 1})):
            w[at] = SPECIAL[(seed + j) % k]
    return w


def _records(n, seed, n_nrn=N_NRN):
    rng = np.random.default_rng(seed)
    return _syn(rng.integers(0, n_nrn, n, dtype=np.uint32), rng.integers(0, n_nrn, n, dtype=np.uint32), _weights(n, seed))


def _brain(n_syn, n_hidden=488, **kw):
    import abnn_amd

    return abnn_amd.Brain(256, 256, n_hidden, n_syn, 100_000, **kw)


def _even_bounds(pops, n_nrn=N_NRN):
    return (np.arange(pops + 1, dtype=np.uint64) * n_nrn // pops).astype(np.uint32)


def _labels_of(bounds, n_nrn=N_NRN):
    """The label plane that states the same partition as `bounds`, none = 0xFFFFFFFF."""
    b = np.asarray(bounds, dtype=np.int64)
    ids = np.arange(n_nrn)
    j = np.searchsorted(b, ids, side="right") - 1
    return np.where((ids >= b[0]) & (ids < b[-1]), j, NONE).astype(np.uint32)


# ---- 1. record-count edges ---------------------------------------------------------------------
# 4096 records are one workgroup iteration (2 x 512 threads x 4 loads): 4095 .. 4097 cross it with and without
# the odd last record, 8193 is two iterations and that record; 63 .. 65 are one wave's lanes.
@pytest.mark.parametrize("n_syn", [1, 2, 3, 63, 64, 65, 4095, 4096, 4097, 8193])
def test_record_count_edges(gpu, n_syn):
    with _brain(n_syn) as b:
        syn = _records(n_syn, n_syn)
        b.upload_synapses(syn)
        back = b.download_synapses()
        assert np.array_equal(back.view(np.uint32), syn.view(np.uint32))
        inner = np.array([100, 100, 400, 640, 900], dtype=np.uint32)  # an empty population, a prefix and a suffix unassigned
        for bounds in (None, inner, _even_bounds(64)):
            for what, weights in ((ALL, None), (("count",), (0.25, 0.9)), (("w",), None), (("count", "p"), (-np.inf, np.inf))):
                got = _against_reference(b, bounds, what=what, weights=weights, syn=back, note=f"n {n_syn}")
                assert got["records"] == n_syn and got["neurons"] == N_NRN
        lab = _labels_of(inner)
        lab[::7] = 4  # == P: no population
        _against_reference(b, labels=lab, pops=4, syn=back, note=f"labels n {n_syn}")


# ---- 2. cell patterns: contention and run heads -------------------------------------------------------
def _cells_to_records(cells, pops, seed):
    """Records whose (pop(src), pop(dst)) follow `cells` = a * P + b under _even_bounds(pops)."""
    bounds = _even_bounds(pops).astype(np.int64)
    rng = np.random.default_rng(seed)
    a, b = cells // pops, cells % pops
    src = bounds[a] + rng.integers(0, 1 << 30, len(cells)) % (bounds[a + 1] - bounds[a])
    dst = bounds[b] + rng.integers(0, 1 << 30, len(cells)) % (bounds[b + 1] - bounds[b])
    return _syn(src.astype(np.uint32), dst.astype(np.uint32), _weights(len(cells), seed))


def _run_pattern(b, cells, pops, seed, note):
    syn = _cells_to_records(np.asarray(cells, dtype=np.int64), pops, seed)
    b.upload_synapses(syn)
    bounds = _even_bounds(pops)
    got = _against_reference(b, bounds, syn=syn, note=note)
    want_count = np.bincount(np.asarray(cells), minlength=pops * pops).reshape(pops, pops)
    assert np.array_equal(got["count"], want_count.astype(np.uint64)), note
    _against_reference(b, labels=_labels_of(bounds), pops=pops, syn=syn, note=note + " labels")
    return got


N_PAT = 8193


def test_every_record_in_one_cell(gpu):
    """The uniform-wave path: P = 1, and the built-in populations with every record hidden -> hidden."""
    with _brain(N_PAT) as b:
        got = _run_pattern(b, np.zeros(N_PAT, dtype=np.int64), 1, 1, "P 1")
        assert got["count"].tolist() == [[N_PAT]]
        rng = np.random.default_rng(2)
        syn = _syn(rng.integers(512, N_NRN, N_PAT, dtype=np.uint32), rng.integers(512, N_NRN, N_PAT, dtype=np.uint32),
                   _weights(N_PAT, 2))
        b.upload_synapses(syn)
        got = _against_reference(b, syn=syn, note="hidden -> hidden")
        assert got["count"].tolist() == [[0, 0, 0], [0, 0, 0], [0, 0, N_PAT]] and got["sizes"].tolist() == [256, 256, 488]


def test_two_cells_alternating_record_by_record(gpu):
    with _brain(N_PAT) as b:
        _run_pattern(b, np.arange(N_PAT) % 2 * 5 + 1, 3, 3, "alternating")  # cells 1 and 6
        _run_pattern(b, np.arange(N_PAT) % 2 * 4095, 64, 4, "alternating corners")  # the first and the last cell


@pytest.mark.parametrize("run", [2, 3, 64, 127, 128, 129])
def test_runs_of_equal_cells(gpu, run):
    """Run heads at lane and wave boundaries: a wave's load holds 128 consecutive records, a lane two."""
    with _brain(N_PAT) as b:
        for pops, ncell in ((3, 9), (64, 4096)):
            k = np.arange(N_PAT) // run
            _run_pattern(b, (k * 2654435761 % (1 << 32)) % ncell, pops, run, f"run {run} P {pops}")
        _run_pattern(b, ((np.arange(N_PAT) + 1) // run) % 9, 3, run + 1000, f"run {run} shifted by one record")


def test_every_record_in_a_different_cell(gpu):
    with _brain(N_PAT) as b:
        got = _run_pattern(b, np.arange(N_PAT) % 4096, 64, 5, "different cells")
        assert int(got["count"].max()) == 3 and int(got["count"].min()) == 2


WHATS = [tuple(k for k, on in zip(ALL, (m & 1, m & 2, m & 4)) if on) for m in range(1, 8)]


@pytest.mark.parametrize("pops", [57, 58, 63, 64])
def test_every_subset_of_what_at_the_lds_limit(gpu, pops):
    """The planes of one launch must fit 64 KiB of LDS: COUNT | W | P fits up to 57 populations, W | P up to
    63; past that the call scans twice.  Every subset of `what` on both partition kinds and every path."""
    with _brain(N_PAT) as b:
        cells = (np.arange(N_PAT) * 2654435761 % (1 << 32)) % (pops * pops)
        cells[:pops * pops] = np.arange(pops * pops)  # every cell at least once, the last one included
        bounds = (np.arange(pops + 1, dtype=np.uint64) * N_NRN // pops).astype(np.uint32)
        lo, hi = bounds[:-1].astype(np.int64), bounds[1:].astype(np.int64)
        rng = np.random.default_rng(pops)
        a, c = cells // pops, cells % pops
        syn = _syn((lo[a] + rng.integers(0, 1 << 30, N_PAT) % (hi[a] - lo[a])).astype(np.uint32),
                   (lo[c] + rng.integers(0, 1 << 30, N_PAT) % (hi[c] - lo[c])).astype(np.uint32), _weights(N_PAT, pops))
        b.upload_synapses(syn)
        lab = _labels_of(bounds)
        for what in WHATS:
            got = _against_reference(b, bounds, what=what, syn=syn, note=f"P {pops}")
            assert got["counted"] == N_PAT and set(got) >= set(what)
            _against_reference(b, labels=lab, pops=pops, what=what, weights=(0.25, 0.9), syn=syn, note=f"P {pops} labels")


def test_two_runs_give_equal_words(gpu):
    from abnn_amd import matrix

    with _brain(200_001, n_hidden=9488) as b:
        b.upload_synapses(_records(200_001, 11, 10_000))
        lab = np.random.default_rng(12).integers(0, 9, 10_000).astype(np.uint32)
        for kw in ({"bounds": _even_bounds(64, 10_000)}, {"labels": lab, "pops": 8}):
            first = matrix.to_words(b.matrix(what=ALL, **kw))
            again = matrix.to_words(b.matrix(what=ALL, **kw))
            assert np.array_equal(first, again)
        _against_reference(b, _even_bounds(64, 10_000), note="200001 records")
        _against_reference(b, labels=lab, pops=8, note="200001 records, labels")


# ---- 3. label planes ------------------------------------------------------------------------------------
def _hip():
    with open("/proc/self/maps") as f:  # the HIP runtime the library loaded, not a second one
        loaded = {line.split()[-1] for line in f if "libamdhip64.so" in line}
    assert len(loaded) == 1, loaded
    hip = C.CDLL(loaded.pop())
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


def _write_raw_records(b, hip, recs):
    """Records that no upload validates, written into the {dst, w} array as abnn_state_ptrs allows."""
    base, nbytes, elem = b.synapse_layout()["arrays"]["dst_w"]
    assert elem == 8
    for k, dst in recs:
        assert (int(k) + 1) * 8 <= nbytes
        rec = np.array([dst, np.array([0.5], dtype=F32).view(np.uint32)[0]], dtype=np.uint32)
        assert hip.hipMemcpy(base + int(k) * 8, rec.ctypes.data, 8, 1) == 0  # hipMemcpyHostToDevice


def test_labels_with_none_values_an_odd_n_nrn_and_ids_that_are_no_neuron(gpu):
    n_nrn, n_syn = 1001, 5001
    hip = _hip()
    with _brain(n_syn, n_hidden=n_nrn - 512) as b:
        assert b.n_neuron() == n_nrn
        syn = _records(n_syn, 21, n_nrn)
        syn["src"][[10, 4000]] = syn["dst"][[10, 4000]] = NONE  # tombstones
        syn["src"][7], syn["dst"][7] = n_nrn - 1, n_nrn - 1     # the last valid id
        b.upload_synapses(syn)
        # a dst that is N_NRN, a dst far above it, and a live record on a tombstone's src code (a src that is no neuron)
        _write_raw_records(b, hip, ((20, n_nrn), (21, 0xFFFFFFFE), (10, 7)))
        back = b.download_synapses()
        assert back["dst"][[20, 21, 10]].tolist() == [n_nrn, 0xFFFFFFFE, 7] and back["src"][10] >= n_nrn
        rng = np.random.default_rng(22)
        for pops in (1, 5, 64):
            lab = rng.integers(0, pops + 3, n_nrn).astype(np.uint32)  # pops .. pops + 2: no population
            lab[rng.integers(0, n_nrn, 50)] = NONE
            lab[[0, 7, n_nrn - 1]] = pops - 1
            clean = lab.copy()
            clean[clean >= pops] = 0  # every neuron assigned: only the ids that are no neuron stay out
            got = _against_reference(b, labels=clean, pops=pops, syn=back, note=f"clean P {pops}")
            assert (got["src_unassigned"], got["dst_unassigned"], got["unassigned"]) == (1, 2, 0)
            assert got["tombstones"] == 1 and got["assigned"] == n_nrn
            got = _against_reference(b, labels=lab, pops=pops, what=("count", "p"), weights=(0.25, 0.9), syn=back,
                                     note=f"P {pops}")
            assert got["assigned"] == int((lab < pops).sum()) < n_nrn
        # the same records under bounds: the run ends clean there too
        got = _against_reference(b, [0, 500, n_nrn], syn=back)
        assert (got["src_unassigned"], got["dst_unassigned"], got["unassigned"]) == (1, 2, 0)


def test_composition_with_hops_and_components_on_one_stream(gpu):
    """hops_enqueue from the inputs, then the matrix with labels_dev pointing at the distance plane inside the
    hops result, on the same stream with no synchronise between; likewise a components label plane with P = 1."""
    import torch

    import abnn_amd
    from abnn_amd import components, hops, matrix

    with abnn_amd.Brain(256, 256, 9489, 60_001, 100_000) as b:  # 10,001 neurons: odd
        b.build_random_graph(3)
        n_nrn = b.n_neuron()
        syn = b.download_synapses()
        warm = torch.zeros(n_nrn, dtype=torch.int32, device="cuda:0")
        b.matrix(labels=warm, pops=1)  # the handle's first LABELS call allocates the scratch: it may synchronise
        hcfg = hops.config((0, 256), 6)
        ccfg = components.config(None, (0.62, np.inf), False, n_nrn)
        h_out = torch.zeros(hops.n_words(hcfg, n_nrn), dtype=torch.int64, device="cuda:0")
        c_out = torch.zeros(components.n_words(ccfg, n_nrn), dtype=torch.int64, device="cuda:0")
        side = torch.cuda.Stream(device=0)
        results = []
        for path in (1, 2):
            _set_path(b, path)
            mh, mc = matrix.config(8, ALL, labels=True), matrix.config(1, ("count", "w"), labels=True)
            mh_out = torch.zeros(matrix.n_words(mh), dtype=torch.int64, device="cuda:0")
            mc_out = torch.zeros(matrix.n_words(mc), dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            b.hops_enqueue(hcfg, h_out.data_ptr(), stream=side)
            b.matrix_enqueue(mh, mh_out.data_ptr(), labels_ptr=h_out.data_ptr() + 8 * hops.plane_offset(hcfg), stream=side)
            b.components_enqueue(ccfg, c_out.data_ptr(), stream=side)
            b.matrix_enqueue(mc, mc_out.data_ptr(), labels_ptr=c_out.data_ptr() + 8 * components.PLANE_AT, stream=side)
            side.synchronize()
            dist = hops.decode(h_out.cpu().numpy().view(np.uint64), hcfg, n_nrn)["dist"]
            labels = components.decode(c_out.cpu().numpy().view(np.uint64), ccfg, n_nrn)["labels"]
            got_h = matrix.decode(mh_out.cpu().numpy().view(np.uint64), mh)
            got_c = matrix.decode(mc_out.cpu().numpy().view(np.uint64), mc)
            _same(got_h, matrix.reference(syn, mh, n_nrn, b.params.base_scale, labels=dist), f"hops path {path}")
            _same(got_c, matrix.reference(syn, mc, n_nrn, b.params.base_scale, labels=labels), f"components path {path}")
            assert got_h["sizes"][0] == 256 and got_h["count"][0, 0] == 0  # layer 0 is the inputs
            assert got_c["sizes"][0] == int((labels == 0).sum()) >= 1  # label 0 only: neuron 0's component
            results.append((got_h, got_c))
        _set_path(b, 0)
        _same(results[0][0], results[1][0])
        _same(results[0][1], results[1][1])


# ---- 4. high ids -------------------------------------------------------------------------------------------
def test_high_neuron_ids(gpu):
    import abnn_amd

    n_nrn = (1 << 24) - 3
    last = n_nrn - 1
    ids = np.array([0, (1 << 18) - 1, 1 << 18, (1 << 18) + 1, 1 << 23, last], dtype=np.uint32)
    rng = np.random.default_rng(9)
    n_syn = 3001
    syn = _syn(ids[rng.integers(0, len(ids), n_syn)], ids[rng.integers(0, len(ids), n_syn)], _weights(n_syn, 9))
    syn["src"][n_syn - 1], syn["dst"][n_syn - 1] = last, last  # the record that no whole load holds
    with abnn_amd.Brain(256, 256, n_nrn - 512, n_syn, 100_000) as b:
        assert b.n_neuron() == n_nrn
        b.upload_synapses(syn)
        back = b.download_synapses()
        assert np.array_equal(back.view(np.uint32), syn.view(np.uint32))
        # every planted id a population of its own, edges exactly at the ids; then an unassigned suffix that holds `last`
        edges = np.array([0, 1, (1 << 18) - 1, 1 << 18, (1 << 18) + 1, (1 << 18) + 2, 1 << 23, (1 << 23) + 1, last, n_nrn],
                         dtype=np.uint32)
        got = _against_reference(b, edges, syn=back, note="high ids")
        assert got["counted"] == n_syn and got["count"][8, 8] >= 1
        got = _against_reference(b, edges[:-1], syn=back, note="last unassigned")
        assert got["counted"] < n_syn and got["unassigned"] >= 1
        got = _against_reference(b, _even_bounds(64, n_nrn), syn=back, note="64 wide")
        assert got["counted"] == n_syn
        lab = np.full(n_nrn, NONE, dtype=np.uint32)
        lab[ids] = np.arange(len(ids))
        got = _against_reference(b, labels=lab, pops=6, syn=back, paths=(1, 2), note="high ids, labels")
        assert got["counted"] == n_syn and got["sizes"].tolist() == [1] * 6
        lab[last] = 6
        got = _against_reference(b, labels=lab, pops=6, syn=back, paths=(1, 2), note="last is none")
        assert got["unassigned"] >= 1 and got["assigned"] == 5


# ---- 5. state and lifetime -------------------------------------------------------------------------------------
def test_tombstones_and_capacity_headroom(gpu):
    """Records past n_syn are never read: live-looking records are written into the headroom."""
    n = 5_000
    syn = _records(n, 3)
    dead = np.random.default_rng(4).choice(n, 500, replace=False)
    syn["src"][dead] = syn["dst"][dead] = NONE
    with _brain(n, syn_capacity=9_000) as b:
        b.upload_synapses(syn)
        hip = _hip()
        _write_raw_records(b, hip, ((n, 5), (n + 1, 600), (8_999, 7)))  # past n_syn: never read
        back = b.download_synapses()
        assert len(back) == n and int((back["dst"] == NONE).sum()) == 500
        got = _against_reference(b, syn=back)
        assert got["records"] == n and got["tombstones"] == 500 and got["counted"] == n - 500
        _against_reference(b, _even_bounds(64), weights=(0.25, 0.9), syn=back)
        _against_reference(b, labels=_labels_of([100, 300, 900]), pops=2, syn=back)


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
    assert before["tombstones"] == 20_000
    b.set_auto_stimulus(0, 256)
    b.encode_traversal(2)  # the second pass runs the structural update: the tombstones are removed
    assert b.n_syn() <= n_syn - 20_000
    after_syn = b.download_synapses()
    assert len(after_syn) == b.n_syn() and not (after_syn["dst"] == NONE).any()
    after = _against_reference(b, syn=after_syn)
    assert after["records"] == b.n_syn() < before["records"] and after["tombstones"] == 0
    _against_reference(b, labels=_labels_of(_even_bounds(16, 3512), 3512), pops=16, weights=(0.2, np.inf), syn=after_syn)
    b.close()


def test_enqueue_between_passes_on_a_side_stream(gpu):
    """The passes' outputs are byte-identical with and without the matrices between them."""
    import torch

    import abnn_amd
    from abnn_amd import matrix

    def make():
        b = abnn_amd.Brain(256, 256, 99_488, 1_000_000, 1_000_000)
        b.build_random_graph(1)
        b.set_auto_stimulus(0, 256)
        return b

    a, twin = make(), make()
    n_nrn = a.n_neuron()
    lab = (np.arange(n_nrn, dtype=np.uint32) * np.uint32(2654435761) >> np.uint32(28)) % np.uint32(10)  # 8, 9: none
    lab_dev = torch.from_numpy(lab.view(np.int32)).to("cuda:0")
    io = matrix.io_bounds(256, 256, 99_488)
    cases = [(matrix.config(3, ALL), io, None), (matrix.config(8, ("count", "p"), labels=True), None, lab),
             (matrix.config(64, ALL, weights=(0.3, 0.9)), _even_bounds(64, n_nrn), None), (matrix.config(3, ALL), io, None)]
    outs = [torch.zeros(matrix.n_words(c), dtype=torch.int64, device="cuda:0") for c, _, _ in cases]
    a.matrix(labels=lab_dev, pops=8)  # the handle's first LABELS call allocates the scratch: it may synchronise
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=0)
    a.encode_traversal(6, stream=side)  # the weights move from the fourth pass
    for path, ((c, bounds, labels), o) in zip((0, 2, 3, 1), zip(cases, outs)):
        _set_path(a, path)
        a.matrix_enqueue(c, o.data_ptr(), bounds=bounds, labels_ptr=None if labels is None else lab_dev.data_ptr(), stream=side)
    a.encode_traversal(2, stream=side)
    side.synchronize()
    twin.encode_traversal(6)
    syn = twin.download_synapses()
    got = [matrix.decode(o.cpu().numpy().view(np.uint64), c) for (c, _, _), o in zip(cases, outs)]
    for (c, bounds, labels), g in zip(cases, got):
        _same(g, matrix.reference(syn, c, n_nrn, a.params.base_scale, bounds=bounds, labels=labels))
    _same(got[0], got[3])
    twin.encode_traversal(2)
    assert a.checksum() == twin.checksum()  # the matrices wrote nothing but their results
    assert np.array_equal(a.download_synapses().view(np.uint32), twin.download_synapses().view(np.uint32))
    assert np.array_equal(a.last_fired(), twin.last_fired()) and a.scalars() == twin.scalars()
    assert a.stats() == twin.stats()
    # refused on the host, before any launch
    ok, out0 = cases[0][0], outs[0].data_ptr()
    for cfg, bounds, labels_ptr, out_ptr in (
            (matrix.config(0), [0], None, out0), (matrix.config(65), list(range(66)), None, out0),  # pops outside 1..64
            (ok, [0, 300, 200, n_nrn], None, out0),        # decreasing bounds
            (ok, [0, 256, 512, n_nrn + 1], None, out0),    # bounds[P] > N_NRN
            (ok, None, None, out0), (ok, io, lab_dev.data_ptr(), out0),  # no partition, both
            (ok, None, lab_dev.data_ptr(), out0),          # labels without the flag
            (cases[1][0], _even_bounds(8, n_nrn), None, outs[1].data_ptr()),  # bounds with the flag
            (cases[1][0], None, lab_dev.data_ptr() + 2, outs[1].data_ptr()),  # a misaligned plane
            (ok, io, None, out0 + 4)):                     # a misaligned result
        with pytest.raises(abnn_amd.AbnnError) as err:
            a.matrix_enqueue(cfg, out_ptr, bounds=bounds, labels_ptr=labels_ptr)
        assert err.value.status == 1
    with pytest.raises(abnn_amd.AbnnError) as err:
        _set_path(a, 5)
    assert err.value.status == 1
    a.close()
    twin.close()


def test_no_records_gives_the_sizes_only(gpu):
    with _brain(0) as b:  # no records: the sizes only
        assert b.n_syn() == 0
        got = _against_reference(b)
        assert got["records"] == 0 and got["sizes"].tolist() == [256, 256, 488] and not got["count"].any()
        got = _against_reference(b, labels=_labels_of([0, 10, 20]), pops=2)
        assert got["sizes"].tolist() == [10, 10] and got["assigned"] == 20


# ---- 6. shards ------------------------------------------------------------------------------------------------
def test_merged_shards_equal_the_unsharded_result(gpu):
    import abnn_amd
    from abnn_amd import matrix
    from abnn_amd.shard import global_events, shard_ranges

    n_syn, events = 10_001, 100_000
    with _brain(n_syn) as whole:
        syn = _records(n_syn, 7)
        whole.upload_synapses(syn)
        ge = global_events(n_syn, events, 2)
        shards = []
        for lo, hi in shard_ranges(n_syn, 2):
            s = abnn_amd.Brain(256, 256, 488, hi - lo, events, syn_offset=lo, global_events=ge)
            s.upload_synapses(syn[lo:hi])
            shards.append(s)
        lab = _labels_of([5, 300, 300, 990])
        for kw in ({"bounds": None}, {"bounds": _even_bounds(64)}, {"labels": lab, "pops": 3}):
            for weights in (None, (0.25, 0.9)):
                want = _against_reference(whole, what=ALL, weights=weights, syn=syn, **kw)
                parts = [s.matrix(what=ALL, weights=weights, **kw) for s in shards]
                assert [p["records"] for p in parts] == [hi - lo for lo, hi in shard_ranges(n_syn, 2)]
                _same(matrix.merge(parts), want, str(kw))
        for s in shards:
            s.close()


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_sharded_brain_matrix_world1(gpu, monkeypatch):
    import torch.distributed as dist

    from abnn_amd.shard import ShardedBrain, TorchComm

    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(_port()))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        sb = ShardedBrain(TorchComm(), 256, 256, 488, 10_000, 100_000, device=0, native=True)
        sb.brain.build_random_graph(1)
        lab = _labels_of([0, 256, 512, 700])
        for kw in ({}, {"bounds": _even_bounds(64), "what": ALL}, {"labels": lab, "pops": 3, "what": ("p",)},
                   {"weights": (0.3, 0.9)}):
            _same(sb.matrix(**kw), sb.brain.matrix(**kw), str(kw))
            ref_kw = {k: v for k, v in kw.items() if k in ("bounds", "labels", "pops", "weights")}
            _same(sb.matrix(**kw), _against_reference(sb.brain, what=kw.get("what", ("count", "w")), **ref_kw), str(kw))
        sb.native.close()
        sb.brain.close()
    finally:
        dist.destroy_process_group()


# ---- 7. the C++ mirrors ----------------------------------------------------------------------------------------
def test_cpp_matrix(gpu):
    from abnn_amd.build import build_matrix_test

    prog = build_matrix_test()
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    lines = r.stdout.strip().splitlines()
    assert lines, (r.returncode, r.stderr[-2000:])
    res = json.loads(lines[-1])
    assert r.returncode == 0 and res["ok"], (res, r.stderr[-2000:])
    assert res["records"] == 100_000 == res["io_counted"] and res["neurons"] == 10_000
    assert 0 < res["hidden_hidden"] < 100_000 and 0 < res["label_counted"] < 100_000


# ---- 8. device memory ---------------------------------------------------------------------------------------------
def test_live_allocations_return_after_destroy(gpu):
    from abnn_amd import _lib

    live = lambda: int(_lib.load().abnn_debug_live_allocations())  # noqa: E731
    base = live()
    b = _brain(5_000)
    b.upload_synapses(_records(5_000, 2))
    created = live()
    b.matrix()
    assert live() == created + 1  # the synchronous call's result; BOUNDS needs no scratch
    lab = _labels_of([0, 500, 1000])
    # a refused call has no side effect: the words are checked before the LABELS scratch is allocated
    import torch

    from abnn_amd import matrix

    cfg = matrix.config(2, labels=True)
    dev = torch.from_numpy(lab.view(np.int32)).to("cuda:0")
    out = np.zeros(matrix.n_words(cfg) + 1, dtype=np.uint64)
    assert _lib.load().abnn_matrix(b._h, C.byref(cfg), None, dev.data_ptr(), out.ctypes.data, matrix.n_words(cfg) + 1) == 1
    assert live() == created + 1
    b.matrix(labels=lab, pops=2)
    first = live()
    assert first == created + 2  # the packed plane
    for path in LABELS_PATHS:
        _set_path(b, path)
        b.matrix(_even_bounds(64), what=ALL)  # a larger result: the buffer grows once, the old one is freed
        b.matrix(labels=lab, pops=2, what=ALL)
    assert live() == first
    b.close()
    assert live() == base
