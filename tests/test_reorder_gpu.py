"""The record reorder on the GPU (abnn.h abnn_reorder_*, csrc/reorder.hip).

Every comparison is Brain.reorder(..., origin=True) followed by
download_synapses() against reorder.reference over the same brain's earlier
download: the records as u32 words, origin and the header equal.  Record-count
edges around the tile and the vector tail, a brain of several tiles per CU, few
workgroups that take several tiles each, key shapes (ties, sorted, reversed,
one byte, all 256 buckets), the special weights, tombstones, the shuffle, PERM
valid and invalid, capacity headroom, the bookkeeping (src mirror, pruning
tally) through passes that follow, the enqueue-only path on a side stream,
shards, the C++ mirror and the learning loop."""
import json
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
U32 = np.uint32
NONE = 0xFFFFFFFF
# NaN of both signs, +-inf, -0.0 / +0.0, a denormal of each sign
SPECIAL_BITS = np.array([0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x00012345,
                         0x80012345], dtype=U32)
BIG = 3_000_001  # 733 tiles over every CU; the last record is in no 16-byte pair
BIG_NRN = 100_512  # 256 + 256 + 100 000: ids at and above 2^16
MULTI = 3 * 4096 + 17  # four tiles, the last one short and odd
SENTINEL = 0x5A5A5A5A5A5A5A5A
KEYS = (("src", False), ("src", True), ("dst", False), ("dst", True), ("w", False), ("w", True), ("random", False),
        ("none", False))


def _tile():
    from abnn_amd import reorder

    return reorder.TILE


def _records(n, seed, n_nrn=1000, tombstones=0):
    """Seeded records with uniform src / dst, weights in [-0.1, 1.1] and the
    special values planted at the first, a middle and the last index;
    ``tombstones``: that many at the first, the last and scattered indices."""
    from abnn_amd import SYN_DTYPE

    rng = np.random.default_rng(seed)
    syn = np.zeros(n, dtype=SYN_DTYPE)
    syn["src"] = rng.integers(0, n_nrn, n, dtype=U32)
    syn["dst"] = rng.integers(0, n_nrn, n, dtype=U32)
    syn["w"] = rng.uniform(-0.1, 1.1, n).astype(F32)
    k = len(SPECIAL_BITS)
    if n >= 3 * k:
        for at in (0, n // 2 - k // 2, n - k):
            syn["w"].view(U32)[at:at + k] = SPECIAL_BITS
    else:
        for j, at in enumerate(sorted({0, n // 2, n - 1} & set(range(n)))):
            syn["w"].view(U32)[at] = SPECIAL_BITS[(seed + j) % k]
    if tombstones and n:
        at = np.unique(np.concatenate([[0, n - 1], rng.integers(0, n, max(tombstones - 2, 0))]))
        syn["src"][at] = syn["dst"][at] = NONE
    return syn


def _brain(n_syn, **kw):
    import abnn_amd

    return abnn_amd.Brain(256, 256, 488, n_syn, 100_000, **kw)


def _big_brain():
    import abnn_amd

    return abnn_amd.Brain(256, 256, 100_000, BIG, 100_000)


def _words(a):
    return np.ascontiguousarray(a).view(U32).reshape(-1, 4)


def _check(b, key, before=None, note="", descending=False, seed=0, perm=None):
    """Brain.reorder(origin=True) and the download after it against the reference
    over the download before it.  Returns (result, download after)."""
    from abnn_amd import reorder

    before = b.download_synapses() if before is None else before
    got = b.reorder(key, descending=descending, seed=seed, origin=True, perm=perm)
    after = b.download_synapses()
    cfg = reorder.config("perm" if perm is not None else key, descending, seed, True)
    want, origin, head = reorder.reference(before, cfg, int(b.dims.syn_offset), perm)
    what = (note, key, descending, seed, len(before))
    assert {k: got[k] for k in reorder.HEADER_KEYS} == head, what
    assert got["origin"].dtype == U32 and got["origin"].shape == (len(before),), what
    bad = np.flatnonzero(got["origin"] != origin)
    assert bad.size == 0, (what, bad[:8].tolist(), got["origin"][bad[:8]].tolist(), origin[bad[:8]].tolist())
    g, w = _words(after), _words(want)
    bad = np.flatnonzero((g != w).any(axis=1))
    assert bad.size == 0, (what, bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist())
    return got, after


# ---- 1. record-count edges ---------------------------------------------------------------------
@pytest.mark.parametrize("n_syn", [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193])
def test_record_count_edges(gpu, n_syn):
    syn = _records(n_syn, n_syn + 1, tombstones=3 if n_syn >= 3 else 0)
    with _brain(n_syn) as b:
        for key, desc in KEYS:
            b.upload_synapses(syn)
            got, after = _check(b, key, before=syn, descending=desc, seed=7 if key == "random" else 0)
            assert got["records"] == n_syn
            t = got["tombstones"]
            assert (after["dst"][n_syn - t:] == NONE).all() and (after["dst"][:n_syn - t] != NONE).all()


def test_few_workgroups_take_several_tiles_each(gpu, monkeypatch):
    """A workgroup carries its offsets from tile to tile only when there are more
    tiles than workgroups: 3 workgroups (ABNN_REORDER_BLOCKS, read when the
    handle is created), so a segment is 2 or 4 tiles; record counts one below,
    at and one above a segment's end, and a last segment that is short."""
    monkeypatch.setenv("ABNN_REORDER_BLOCKS", "3")
    tile = _tile()
    for n_syn in (4 * tile - 1, 4 * tile, 4 * tile + 1, 6 * tile + 1, 10 * tile + 1):
        syn = _records(n_syn, 3, tombstones=40)
        with _brain(n_syn) as b:
            for key, desc in (("dst", False), ("w", True), ("random", False), ("src", False)):
                b.upload_synapses(syn)
                _check(b, key, before=syn, descending=desc, seed=11 if key == "random" else 0, note="3 workgroups")


# ---- 2. a brain of 733 tiles ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """One brain of 3 000 001 records over 100 512 neurons (ids at and above
    2^16) with 1000 tombstones; every test uploads the records it wants."""
    syn = _records(BIG, 5, BIG_NRN, tombstones=1000)
    syn.setflags(write=False)
    b = _big_brain()
    yield b, syn
    b.close()


@pytest.mark.parametrize("key, desc", [("src", False), ("dst", True), ("w", False), ("random", False), ("none", False)])
def test_big_brain(gpu, big, key, desc):
    b, syn = big
    assert BIG > 700 * _tile() and BIG % 2 == 1 and int(syn["src"][syn["src"] != NONE].max()) >= 1 << 16
    b.upload_synapses(syn)
    got, after = _check(b, key, before=syn, descending=desc, seed=3 if key == "random" else 0, note="big")
    t = got["tombstones"]
    assert t == int((syn["dst"] == NONE).sum()) > 900 and (after["dst"][BIG - t:] == NONE).all()
    if key == "none":  # nothing but the tombstones moved: the live records keep their order
        live = syn[syn["dst"] != NONE]
        assert np.array_equal(_words(after[:BIG - t]), _words(live))


def test_big_brain_long_runs_of_ties(gpu, big):
    """3M records over 1000 neurons: 3000 equal keys per neuron, on both id keys."""
    b, _ = big
    syn = _records(BIG, 9, 1000)
    for key in ("dst", "src"):
        b.upload_synapses(syn)
        got, after = _check(b, key, before=syn, note="ties")
        assert got["tombstones"] == 0 and (np.diff(after[key].astype(np.int64)) >= 0).all()


# ---- 3. key shapes -------------------------------------------------------------------------------
def _shape(kind):
    """MULTI records over 1000 neurons whose dst (and, for the w shapes, w) has the shape `kind`."""
    syn = _records(MULTI, 21)
    rng = np.random.default_rng(22)
    k = np.arange(MULTI)
    if kind == "equal":
        syn["dst"] = 7
    elif kind == "sorted":
        syn["dst"] = np.sort(syn["dst"])
    elif kind == "reversed":
        syn["dst"] = np.sort(syn["dst"])[::-1]
    elif kind == "alternating":
        syn["dst"] = np.where(k & 1, 900, 3)
    elif kind == "lowest byte":
        syn["dst"] = 256 + rng.integers(0, 256, MULTI)
    elif kind == "highest used byte":
        syn["dst"] = rng.integers(0, 4, MULTI) << 8 | 0x5A  # 0x05A, 0x15A, 0x25A, 0x35A
    elif kind == "256 buckets beside one":
        syn["dst"][:4096] = rng.permutation(4096) % 256  # tile 0 hits every bucket of the lowest digit
        syn["dst"][4096:8192] = 5                        # tile 1 a single one
    elif kind == "w equal":
        syn["w"] = F32(0.375)
    elif kind == "w lowest byte":
        syn["w"].view(U32)[:] = 0x3E800000 | rng.integers(0, 256, MULTI).astype(U32)
    elif kind == "w highest byte":
        syn["w"].view(U32)[:] = (rng.integers(0, 256, MULTI).astype(U32) << 24) | U32(0x00345678)  # NaNs among them
    else:
        raise AssertionError(kind)
    return syn


@pytest.mark.parametrize("kind", ["equal", "sorted", "reversed", "alternating", "lowest byte", "highest used byte",
                                  "256 buckets beside one", "w equal", "w lowest byte", "w highest byte"])
def test_key_shapes(gpu, kind):
    syn = _shape(kind)
    key = "w" if kind.startswith("w ") else "dst"
    with _brain(MULTI) as b:
        for desc in (False, True):
            b.upload_synapses(syn)
            got, after = _check(b, key, before=syn, descending=desc, note=kind)
            if kind in ("equal", "w equal") or (kind == "sorted" and not desc):  # stability: nothing moves
                assert got["moved"] == 0 and np.array_equal(got["origin"], np.arange(MULTI, dtype=U32))
            if kind == "reversed" and not desc:
                assert got["moved"] > MULTI // 2
            if kind == "alternating":
                half = MULTI // 2 + (MULTI & 1 if not desc else 0)  # the records of the value that comes first
                assert (np.diff(got["origin"][:half].astype(np.int64)) == 2).all()


def test_neuron_ids_above_2_18(gpu):
    """src and dst ids on both sides of 2^18 and 2^23 (high_id_helpers.fixed_ids:
    every id class's first and last id): the src code's folded classes decode
    to the interchange value the key is, and the third digit is in use."""
    import abnn_amd
    from high_id_helpers import fixed_ids

    n_nrn = (1 << 23) + 4096
    ids = fixed_ids(n_nrn)
    assert (ids >= 1 << 18).sum() > 30 and (ids >= 1 << 23).sum() >= 2
    rng = np.random.default_rng(4)
    syn = _records(MULTI, 31)
    syn["src"] = ids[rng.integers(0, len(ids), MULTI)]
    syn["dst"] = ids[rng.integers(0, len(ids), MULTI)]
    syn["src"][[1, MULTI - 2]] = syn["dst"][[1, MULTI - 2]] = NONE
    with abnn_amd.Brain(256, 256, n_nrn - 512, MULTI, 100_000) as b:
        for key, desc in (("src", False), ("src", True), ("dst", False), ("dst", True)):
            b.upload_synapses(syn)
            got, after = _check(b, key, before=syn, descending=desc, note="high ids")
            live = after[key][:MULTI - 2].astype(np.int64)
            assert (np.diff(live) <= 0).all() if desc else (np.diff(live) >= 0).all()


# ---- 4. the special weights --------------------------------------------------------------------------
@pytest.mark.parametrize("n_syn", [MULTI, 100_001])
def test_special_weights(gpu, n_syn):
    from abnn_amd import reorder

    syn = _records(n_syn, 41)
    with _brain(n_syn) as b:
        for desc in (False, True):
            b.upload_synapses(syn)
            got, after = _check(b, "w", before=syn, descending=desc, note="special weights")
            bits = after["w"].view(U32)
            key = bits ^ np.where(bits >> U32(31), U32(0xFFFFFFFF), U32(0x80000000)).astype(U32)
            d = np.diff(key.astype(np.int64))
            assert (d <= 0).all() if desc else (d >= 0).all()
            first, last = (bits[0], bits[-1]) if not desc else (bits[-1], bits[0])
            assert first == 0xFFC00000 and last == 0x7FC00000  # the NaNs at the two ends, by their bits
            zeros = np.flatnonzero((bits & U32(0x7FFFFFFF)) == 0)
            minus = bits[zeros] == 0x80000000
            assert minus.sum() == 3 and (minus[:3].all() if not desc else minus[-3:].all())  # -0.0 < +0.0
        assert reorder.inverse(got["origin"])[got["origin"]].tolist() == list(range(n_syn))


# ---- 5. tombstones ------------------------------------------------------------------------------------
def test_tombstones_are_last_and_in_order(gpu):
    n_syn = MULTI
    syn = _records(n_syn, 51, tombstones=300)
    syn["w"][syn["dst"] == NONE] = np.random.default_rng(1).uniform(-5, 5, int((syn["dst"] == NONE).sum())).astype(F32)
    dead = np.flatnonzero(syn["dst"] == NONE)
    assert dead[0] == 0 and dead[-1] == n_syn - 1 and len(dead) > 250
    with _brain(n_syn) as b:
        for key, desc in KEYS:
            b.upload_synapses(syn)
            got, after = _check(b, key, before=syn, descending=desc, seed=5 if key == "random" else 0, note="tombstones")
            t = len(dead)
            assert got["tombstones"] == t
            assert np.array_equal(got["origin"][n_syn - t:], dead.astype(U32))  # last, in their old order
            assert np.array_equal(_words(after[n_syn - t:])[:, :3], _words(syn[dead])[:, :3])  # their weights stay theirs
            if key == "none":  # nothing else moved
                assert np.array_equal(got["origin"][:n_syn - t], np.flatnonzero(syn["dst"] != NONE).astype(U32))
        # only tombstones, and none
        only = syn.copy()
        only["src"] = only["dst"] = NONE
        for key in ("w", "none", "random"):
            b.upload_synapses(only)
            got, _ = _check(b, key, before=only, seed=1 if key == "random" else 0, note="only tombstones")
            assert got["moved"] == 0 and got["tombstones"] == n_syn
        clean = _records(n_syn, 52)
        b.upload_synapses(clean)
        got, _ = _check(b, "none", before=clean, note="no tombstone")
        assert got["moved"] == 0 and got["tombstones"] == 0


# ---- 6. the shuffle ------------------------------------------------------------------------------------
def test_random_is_a_seeded_shuffle(gpu):
    import abnn_amd
    from abnn_amd import census
    from abnn_amd.shard import global_events

    n_syn = 100_001
    with _brain(n_syn) as b:
        b.build_random_graph(1)
        first = b.download_synapses()
        before, sum0 = census.to_words(b.census(64, -0.5, 1.5, dst=(256, 256))), b.checksum()
        origins = []
        for seed in (1, 0xDEADBEEFCAFEF00D):
            b.upload_synapses(first)
            got, after = _check(b, "random", before=first, seed=seed, note="seeds")
            origins.append(got["origin"])
            assert got["moved"] > 0.99 * n_syn
            # the multiset is preserved: the census is word for word the same; the order is not
            assert np.array_equal(census.to_words(b.census(64, -0.5, 1.5, dst=(256, 256))), before)
            assert b.checksum() != sum0
        assert (origins[0] != origins[1]).mean() > 0.99
    # a handle far into a graph: the keys are those of the global indices
    ge = global_events(3 * n_syn, 100_000, 3)
    with abnn_amd.Brain(256, 256, 488, 10_000, 100_000, syn_offset=12_345, global_events=ge) as s:
        s.upload_synapses(first[:10_000])
        got, _ = _check(s, "random", before=first[:10_000], seed=1, note="syn_offset")
        assert got["syn_offset"] == 12_345 and got["moved"] > 9_900


# ---- 7. PERM ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_syn", [MULTI, 100_001])
def test_perm_undoes_a_reorder_and_refuses_what_is_no_permutation(gpu, n_syn):
    from abnn_amd import reorder

    syn = _records(n_syn, 61, tombstones=25)
    with _brain(n_syn) as b:
        b.upload_synapses(syn)
        first = b.download_synapses()
        got, sorted_ = _check(b, "dst", before=first, note="by dst")
        back, again = _check(b, None, before=sorted_, perm=reorder.inverse(got["origin"]), note="the inverse")
        assert np.array_equal(_words(again), _words(first)) and back["moved"] == got["moved"] and back["invalid"] == 0
        assert back["tombstones"] == int((syn["dst"] == NONE).sum()) > 20  # counted, not moved to the end
        good = np.random.default_rng(2).permutation(n_syn).astype(U32)
        for name, bad, count in (("one repeat", {n_syn // 2: good[0]}, 1), ("an entry equal to n", {5: n_syn}, 1),
                                 ("both, and 0xFFFFFFFF", {0: good[1], n_syn - 1: n_syn, 7: NONE}, 3)):
            perm = good.copy()
            for at, v in bad.items():
                perm[at] = v
            res, after = _check(b, None, before=first, perm=perm, note=name)
            assert res["invalid"] == count and res["moved"] == 0, name
            assert np.array_equal(res["origin"], np.arange(n_syn, dtype=U32)), name
            assert np.array_equal(_words(after), _words(first)), name  # exactly as they were
        res, after = _check(b, None, before=first, perm=good, note="a valid perm")
        assert res["invalid"] == 0 and np.array_equal(_words(after), _words(first[good]))


# ---- 8. capacity headroom ----------------------------------------------------------------------------------
def _hip():
    import ctypes as C

    with open("/proc/self/maps") as f:  # the HIP runtime the library loaded, not a second one
        loaded = {line.split()[-1] for line in f if "libamdhip64.so" in line}
    assert len(loaded) == 1, loaded
    hip = C.CDLL(loaded.pop())
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


def test_records_past_n_syn_are_neither_read_nor_written(gpu):
    """syn_capacity > n_syn: a sentinel pattern written past n_syn in the three
    record arrays (through abnn_synapse_layout) is intact after every key."""
    n_syn, cap = 5_001, 9_000
    syn = _records(n_syn, 71, tombstones=10)
    hip = _hip()
    with _brain(n_syn, syn_capacity=cap) as b:
        lay = b.synapse_layout()["arrays"]
        pats = {}
        for name, eb in (("src_code_lo", 2), ("src_code_hi", 1), ("dst_w", 8)):
            base, nbytes, elem = lay[name]
            assert elem == eb and nbytes >= cap * eb
            pat = np.random.default_rng(eb).integers(1, 255, (cap - n_syn) * eb, dtype=np.uint8)
            assert hip.hipMemcpy(base + n_syn * eb, pat.ctypes.data, pat.size, 1) == 0  # hipMemcpyHostToDevice
            pats[name] = (base + n_syn * eb, pat)
        for key, desc in KEYS:
            b.upload_synapses(syn)
            _check(b, key, before=syn, descending=desc, seed=3 if key == "random" else 0, note="headroom")
        _check(b, None, before=b.download_synapses(), perm=np.arange(n_syn, dtype=U32)[::-1].copy(), note="headroom")
        for name, (ptr, pat) in pats.items():
            back = np.zeros_like(pat)
            assert hip.hipMemcpy(back.ctypes.data, ptr, pat.size, 2) == 0  # hipMemcpyDeviceToHost
            assert np.array_equal(back, pat), name


# ---- 9. the bookkeeping: passes after a reorder ---------------------------------------------------------------
def _smoke_brain(**kw):
    import abnn_amd

    b = abnn_amd.Brain(256, 256, 99_488, 1_000_000, 1_000_000, **kw)
    b.build_random_graph(1)
    b.set_auto_stimulus(0, 256)
    return b


def _plant_tombstones(b, count):
    syn = b.download_synapses()
    at = np.unique(np.concatenate([[0, len(syn) - 1], np.random.default_rng(8).integers(0, len(syn), count)]))
    syn["src"][at] = syn["dst"][at] = NONE
    b.upload_synapses(syn)
    return len(at)


@pytest.mark.parametrize("variant", ["sweep", "random", "structural"])
def test_passes_after_a_reorder_equal_passes_over_the_uploaded_reference(gpu, variant):
    """Brain A runs 3 passes, reorders by dst on the device and runs 5 more.
    Brain B runs the same 3 passes (so that it also holds what the passes keep
    outside the records: the grown records that wait for the structural update),
    then gets reorder.reference of A's pre-reorder download by upload_synapses,
    plus A's timestamps and scalars, and runs the same 5 passes.  Random mode
    picks through the src mirror: it was rebuilt.  `structural`: tombstones
    exist at the reorder and a structural update falls inside the 5 passes: the
    tally was recounted, and the update removes exactly them."""
    import abnn_amd
    from abnn_amd import reorder

    kw = {}
    if variant == "random":
        kw = dict(mode=abnn_amd._lib.MODE_RANDOM)
    elif variant == "structural":
        kw = dict(syn_capacity=1_300_000, seed=13, w_prune=0.105, p_new=0.35, w_init=0.5, compact_every=4)
    a, b = _smoke_brain(**kw), _smoke_brain(**kw)
    try:
        planted = 0
        if variant == "structural":
            planted = _plant_tombstones(a, 5_000)
            assert _plant_tombstones(b, 5_000) == planted
        a.encode_traversal(3)
        b.encode_traversal(3)
        before = a.download_synapses()
        assert np.array_equal(_words(before), _words(b.download_synapses()))
        got = a.reorder("dst")
        assert got["records"] == len(before) and got["moved"] > len(before) // 2 and got["tombstones"] >= planted
        want, _, head = reorder.reference(before, reorder.config("dst"))
        assert {k: got[k] for k in reorder.HEADER_KEYS} == head
        b.upload_synapses(want)
        b.set_last_fired(a.last_fired())
        b.set_last_visited(a.last_visited())
        sc = a.scalars()
        b.set_scalars(sc["clock"], sc["reward"], sc["rbar"], sc["pass_index"])
        a.encode_traversal(5)
        b.encode_traversal(5)
        assert a.n_syn() == b.n_syn()
        ga, gb = a.download_synapses(), b.download_synapses()
        bad = np.flatnonzero((_words(ga) != _words(gb)).any(axis=1))
        assert bad.size == 0, (variant, bad[:8].tolist(), _words(ga)[bad[:8]].tolist(), _words(gb)[bad[:8]].tolist())
        assert np.array_equal(a.last_fired(), b.last_fired()) and np.array_equal(a.last_visited(), b.last_visited())
        assert a.scalars() == b.scalars() and a.stats() == b.stats()
        assert a.stats()["fired"] > 0
        assert not np.array_equal(_words(ga)[:, 2], _words(want)[:len(ga), 2])  # the passes moved the weights
        if variant == "structural":
            assert a.structural_updates() == b.structural_updates() == 2  # after pass 4 and pass 8
            assert not (ga["dst"] == NONE).any()  # the last pass ended with an update: every tombstone is gone
            assert a.n_syn() != len(before)
    finally:
        a.close()
        b.close()


# ---- 10. the enqueue-only path ------------------------------------------------------------------------------
def test_enqueue_between_passes_on_a_side_stream(gpu):
    import torch

    from abnn_amd import reorder

    a, twin = _smoke_brain(), _smoke_brain()
    try:
        n_syn = a.n_syn()
        cfgs = [reorder.config("dst", origin=True), reorder.config("random", seed=9)]
        outs = [torch.full((reorder.n_words(c, n_syn) + 16,), SENTINEL, dtype=torch.int64, device="cuda:0") for c in cfgs]
        assert a.reorder("none")["moved"] == 0  # the first reorder allocates the handle's scratch
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=0)
        done = torch.cuda.Event()
        a.encode_traversal(4, stream=side)
        a.reorder_enqueue(cfgs[0], None, outs[0].data_ptr(), stream=side)
        a.encode_traversal(2, stream=side)
        a.reorder_enqueue(cfgs[1], None, outs[1].data_ptr(), stream=side)
        a.encode_traversal(2, stream=side)
        done.record(side)
        done.synchronize()  # ordered by the event alone
        twin.encode_traversal(4)
        for k, (c, o) in enumerate(zip(cfgs, outs)):
            w = o.cpu().numpy().view(np.uint64)
            words = reorder.n_words(c, n_syn)
            assert (w[words:] == SENTINEL).all(), "written past abnn_reorder_words"
            got = reorder.decode(w[:words], c)
            before = twin.download_synapses()
            want = twin.reorder(c.key, seed=int(c.seed), origin=bool(c.flags & 2))
            assert {h: got[h] for h in reorder.HEADER_KEYS} == {h: want[h] for h in reorder.HEADER_KEYS}
            ref, origin, head = reorder.reference(before, c)
            assert {h: got[h] for h in reorder.HEADER_KEYS} == head
            if k == 0:
                assert np.array_equal(got["origin"], origin) and np.array_equal(want["origin"], origin)
            assert np.array_equal(_words(twin.download_synapses()), _words(ref))
            twin.encode_traversal(2)
        assert a.checksum() == twin.checksum()
        assert np.array_equal(a.last_fired(), twin.last_fired()) and a.scalars() == twin.scalars()
        assert a.stats() == twin.stats()
    finally:
        a.close()
        twin.close()


# ---- 11. shards ---------------------------------------------------------------------------------------------
def test_sharded_brain_reorders_each_slice(gpu):
    from abnn_amd import reorder
    from abnn_amd.shard import LocalGroup, ShardedBrain, shard_ranges

    n_syn = 20_001
    g = LocalGroup(2)
    sbs = [ShardedBrain(g.comm(r, 0), 256, 256, 488, n_syn, 100_000, device=0) for r in range(2)]
    try:
        whole = _records(n_syn, 81, tombstones=20)
        cfg = reorder.config("random", seed=17, origin=True)
        _, k_whole = reorder.keys(whole, cfg, 0)
        for sb, (lo, hi) in zip(sbs, shard_ranges(n_syn, 2)):
            assert int(sb.brain.dims.syn_offset) == lo and sb.brain.n_syn() == hi - lo
            sb.brain.upload_synapses(whole[lo:hi])
            got = sb.reorder("random", seed=17, origin=True)
            want, origin, head = reorder.reference(whole[lo:hi], cfg, lo)
            assert {k: got[k] for k in reorder.HEADER_KEYS} == head and head["syn_offset"] == lo
            assert np.array_equal(got["origin"], origin)
            assert np.array_equal(_words(sb.brain.download_synapses()), _words(want))
            # the slice's keys are the unsharded brain's for the same global indices
            assert np.array_equal(reorder.keys(whole[lo:hi], cfg, lo)[1], k_whole[lo:hi])
    finally:
        for sb in sbs:
            sb.brain.close()
        g.close()


# ---- 12. error statuses, release ------------------------------------------------------------------------------
def test_error_statuses_and_release(gpu):
    import torch

    import abnn_amd
    from abnn_amd import reorder

    n_syn = 1_000
    out = torch.zeros(8 + n_syn, dtype=torch.int64, device="cuda:0")
    perm = torch.arange(n_syn, dtype=torch.int32, device="cuda:0")
    with _brain(n_syn) as b:
        b.build_random_graph(1)
        first = b.download_synapses()
        bad_flag = reorder.config("dst")
        bad_flag.flags = 8
        bad_key = reorder.config("dst")
        bad_key.key = 9
        seeded = reorder.config("w")
        seeded.seed = 1
        for cfg, p in ((bad_flag, None), (bad_key, None), (seeded, None), (reorder.config("none", descending=True), None),
                       (reorder.config("perm"), None), (reorder.config("dst"), perm.data_ptr())):
            with pytest.raises(abnn_amd.AbnnError) as err:
                b.reorder_enqueue(cfg, p, out.data_ptr())
            assert err.value.status == 1
        for kw in (dict(key="random", descending=True), dict(key="src", seed=3)):
            with pytest.raises(abnn_amd.AbnnError) as err:
                b.reorder(**kw)
            assert err.value.status == 1, kw
        torch.cuda.synchronize()
        assert not out.cpu().numpy().any()  # a refused reorder writes nothing
        assert np.array_equal(_words(b.download_synapses()), _words(first))
        b.reorder_enqueue(reorder.config("perm", origin=True), perm.data_ptr(), out.data_ptr())  # the identity, from device memory
        b.synchronize()
        got = reorder.decode(out.cpu().numpy().view(np.uint64)[:8 + n_syn // 2], reorder.config("perm", origin=True))
        assert got["moved"] == 0 and got["invalid"] == 0 and np.array_equal(got["origin"], np.arange(n_syn, dtype=U32))
        b.reorder_release()  # the next reorder allocates the scratch again
        b.reorder_release()
        _check(b, "w", before=first, note="after release")


# ---- 13. the C++ mirror ------------------------------------------------------------------------------------------
def test_cpp_reorder(gpu):
    from abnn_amd.build import build_reorder_test

    prog = build_reorder_test()
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    lines = r.stdout.strip().splitlines()
    assert lines, (r.returncode, r.stderr[-2000:])
    res = json.loads(lines[-1])
    assert r.returncode == 0 and res["ok"], (res, r.stderr[-2000:])
    assert res["records"] == 100_001 and res["cases"] == 7 and res["moved"] > 100_001


# ---- 14. the learning loop ------------------------------------------------------------------------------------------
def test_learning_loop_runs_across_a_reorder(gpu):
    from abnn_amd import LearnEngine, reorder

    rng = np.random.default_rng(3)
    with _smoke_brain() as b:
        with LearnEngine(b) as eng:
            eng.run(rng.random((3, 256)).astype(F32), rng.random((3, 256)).astype(F32))
            b.synchronize()
            before = b.download_synapses()
            got = b.reorder("src", origin=True)
            want, origin, head = reorder.reference(before, reorder.config("src", origin=True))
            assert {k: got[k] for k in reorder.HEADER_KEYS} == head and np.array_equal(got["origin"], origin)
            assert np.array_equal(_words(b.download_synapses()), _words(want))
            passes = b.scalars()["pass_index"]
            eng.run(rng.random((3, 256)).astype(F32), rng.random((3, 256)).astype(F32))
            b.synchronize()
            assert b.scalars()["pass_index"] > passes and b.n_syn() == len(before)
