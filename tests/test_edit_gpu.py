"""The synapse edit on the GPU (abnn.h abnn_edit_*, csrc/edit.hip).

Every comparison is Brain.edit (or edit_enqueue into a prefilled torch buffer)
followed by download_synapses() against edit.reference over the download taken
before: all four u32 of every record equal, the headers equal.  Record-count
edges around the 16-byte pair and the workgroup iteration, a brain of many
iterations per workgroup, few workgroups that loop (a child process), kill
adjacency inside a group of eight and across a tally chunk at every width of
the src code, edit-then-traverse against upload-then-traverse in both modes,
the structural update's tally, the SCALE planes and scale_inputs, the
enqueue-only path, capacity headroom, refusals, shards and the C++ mirror."""
import ctypes as C
import hashlib
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
NONE = 0xFFFFFFFF
INF = float("inf")
SPECIAL = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-40, 0.25, 0.75, 0.7499999, 0.25000003], dtype=F32)
BIG = 3_000_001  # 733 workgroup iterations; the last record is in no 16-byte pair
BIG_NRN = 100_512
USED_NRN = 100_000
SENTINEL = 0x5A5A5A5A5A5A5A5A
CHUNK = 4096  # engine.h kCompactChunk = one workgroup iteration of k_edit
SMALL_CONFIGS = (dict(), dict(dst=(256, 256)), dict(src=(0, 500)), dict(src=(100, 600), dst=(300, 600)),
                 dict(src=(0, 100), dst=(900, 100), any=True), dict(dst=(999, 1), any=True),
                 dict(weights=(0.25, 0.75)), dict(src=(0, 500), weights=(0.25, INF)),
                 dict(src=(0, 300), dst=(0, 300), weights=(-INF, 0.25), any=True))
OPS = {"set": dict(b=0.625), "affine": dict(a=-1.5, b=0.125), "scale_dst": dict(), "scale_src": dict(),
       "draw": dict(a=-0.25, b=0.5, seed=0xC0FFEE), "kill": dict()}


def _records(n, seed, n_nrn=1000):
    """The select tests' records: uniform src / dst, weights in [-0.1, 1.1] and
    the special values planted at the first, a middle and the last index."""
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
    elif n:
        for j, at in enumerate(sorted({0, n // 2, n - 1})):
            syn["w"][at] = SPECIAL[(seed + j) % k]
    return syn


def _big_records():
    syn = _records(BIG, 5, USED_NRN)
    syn["dst"][[0, BIG - 1]] = 100_500
    last = (BIG - 1) // CHUNK * CHUNK
    syn["dst"][last + 1:BIG - 1:3] = 100_501
    return syn


BIG_EDITS = (("affine", dict(dst=(100_500, 1), a=2.0, b=0.5)),       # the first and the last record only
             ("kill", dict(dst=(100_501, 1))),                        # every third record of the last 4096 only
             ("affine", dict(a=0.5, b=0.0625, clamp=(0.0, 0.5))))    # every record


def _brain(n_syn, **kw):
    import abnn_amd

    return abnn_amd.Brain(256, 256, 488, n_syn, 100_000, **kw)


def _plane(rng, m):
    return rng.uniform(0.25, 1.75, m).astype(F32)


def _same_records(got, want, what=""):
    g, w = got.view(np.uint32).reshape(-1, 4), want.view(np.uint32).reshape(-1, 4)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero((g != w).any(axis=1))
    assert bad.size == 0, (what, bad.size, bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist())


def _edit(brain, op, before=None, plane=None, note="", **kw):
    """Brain.edit against the reference over the download taken before; returns
    (the new download, the header)."""
    from abnn_amd import edit

    before = brain.download_synapses() if before is None else before
    cfg = edit.config(op, **kw)
    want, head = edit.reference(before, cfg, brain.n_neuron(), int(brain.dims.syn_offset), plane)
    got = brain.edit(op, plane=plane, **kw)
    after = brain.download_synapses()
    what = f"{note} {op} {kw}"
    assert got == head, (what, got, head)
    _same_records(after, want, what)
    return after, got


def _readers_agree(b, syn, note=""):
    """census / select / degrees of the brain against their references on `syn`."""
    from abnn_amd import census, degree, select

    n_nrn = b.n_neuron()
    got = b.census(8, -0.5, 1.5, dst=(200, 400))
    want = census.reference(syn, census.config(8, -0.5, 1.5, None, (200, 400)))
    assert census.to_words(got).tolist() == census.to_words(want).tolist(), note
    cfg = select.config(src=(0, 600), weights=(0.1, 0.9))
    n = int(select.matches(syn, cfg).sum())
    got, want = b.select(src=(0, 600), weights=(0.1, 0.9), capacity=n), select.reference(syn, cfg, n, n_nrn)
    assert select.to_words(got).tolist() == select.to_words(want).tolist(), note
    got, want = b.degrees((100, 500)), degree.reference(syn, degree.config((100, 500)), n_nrn)
    assert degree.to_words(got).tolist() == degree.to_words(want).tolist(), note


# ---- 1. record-count edges ---------------------------------------------------------------------
@pytest.mark.parametrize("n_syn", [0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 8193, 10_000])
def test_record_count_edges(gpu, n_syn):
    import abnn_amd
    from abnn_amd import edit

    rng = np.random.default_rng(n_syn)
    with _brain(n_syn) as b:
        syn = _records(n_syn, 1)
        if n_syn > 40:
            syn["src"][5::13] = syn["dst"][5::13] = NONE  # tombstones
        for op, params in OPS.items():
            b.upload_synapses(syn)
            now = b.download_synapses()
            _same_records(now, syn)
            for kw in SMALL_CONFIGS:
                plane = None
                if op.startswith("scale"):
                    if kw.get("any"):
                        with pytest.raises(abnn_amd.AbnnError):
                            b.edit(op, plane=_plane(rng, 1000), **kw)
                        continue
                    key = kw.get("dst" if op == "scale_dst" else "src")
                    plane = _plane(rng, key[1] if key else 1000)
                for clamp in (None, (0.0, 0.5)):
                    if op == "kill" and clamp:
                        continue
                    now, head = _edit(b, op, before=now, plane=plane, note=f"n {n_syn}", clamp=clamp, **params, **kw)
                    assert head["records"] == n_syn and head["killed"] == (head["matched"] if op == "kill" else 0)
                    _readers_agree(b, now, f"n {n_syn} {op} {kw}")
        b.upload_synapses(syn)
        assert b.edit("set", b=1.0, dst=(999, 1), weights=(5.0, 6.0)) == dict(
            zip(edit.KEYS, (n_syn, int((syn["dst"] == NONE).sum()), 0, 0, 0, 0)))
        _same_records(b.download_synapses(), syn)


# ---- 2. a brain of 733 workgroup iterations -------------------------------------------------------
def _run_big(b):
    """BIG_EDITS on a brain holding _big_records(): the headers and the download."""
    heads = []
    for op, kw in BIG_EDITS:
        heads.append(b.edit(op, **kw))
    return heads, b.download_synapses()


def test_big_brain(gpu):
    import abnn_amd
    from abnn_amd import edit

    syn = _big_records()
    assert BIG > 700 * CHUNK and BIG % 2 == 1
    want, heads = syn, []
    for op, kw in BIG_EDITS:
        want, head = edit.reference(want, edit.config(op, **kw), BIG_NRN)
        heads.append(head)
    assert [h["matched"] for h in heads] == [2, heads[1]["killed"], BIG - heads[1]["killed"]]
    last = (BIG - 1) // CHUNK * CHUNK
    assert 100 < heads[1]["killed"] == len(range(last + 1, BIG - 1, 3))
    with abnn_amd.Brain(256, 256, 100_000, BIG, 100_000) as b:
        b.upload_synapses(syn)
        got_heads, got = _run_big(b)
        assert got_heads == heads
        _same_records(got, want)
    digest = hashlib.sha256(want.tobytes()).hexdigest()
    for blocks in ("1", "3"):  # few workgroups loop over the 733 tiles (read when the handle is created)
        env = dict(os.environ, ABNN_EDIT_BLOCKS=blocks)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "big"], capture_output=True, text=True,
                           timeout=300, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        res = json.loads(r.stdout.strip().splitlines()[-1])
        assert res["heads"] == heads and res["sha256"] == digest, (blocks, res)


# ---- 3. kill adjacency ----------------------------------------------------------------------------
def _kill_pattern(n):
    """Record indices to kill: per aligned group of eight one of the patterns
    (one alone, a pair's both, its first, its second, four in a row, all but
    one), and a run across the 4096 boundary."""
    groups = ([3], [0, 1], [2], [5], [2, 3, 4, 5], [0, 1, 2, 4, 5, 6, 7], [0, 1, 2, 3, 4, 5, 6], [6, 7], [1, 2])
    idx = []
    for g, pat in enumerate(groups):
        for base in (16 * g, 2048 + 16 * g, CHUNK + 16 * g):
            idx += [base + p for p in pat]
    idx += list(range(CHUNK - 3, CHUNK + 3)) + list(range(2 * CHUNK - 1, 2 * CHUNK + 2)) + [n - 1, n - 3]
    return np.unique([i for i in idx if i < n])


@pytest.mark.parametrize("around", [1000, 1 << 16, 1 << 18, 1 << 23])
@pytest.mark.parametrize("mode", [0, 1])
def test_kill_adjacency(gpu, around, mode):
    import abnn_amd
    from abnn_amd import SYN_DTYPE

    n_hidden = max(around + 600, 1000) - 512
    n_nrn, n = 512 + n_hidden, 3 * CHUNK - 1
    rng = np.random.default_rng(around)
    ids = np.clip(around + rng.integers(-500, 500, n), 0, n_nrn - 2).astype(np.uint32)
    syn = np.zeros(n, dtype=SYN_DTYPE)
    syn["src"], syn["dst"] = ids, np.clip(ids[::-1] + 1, 0, n_nrn - 2)
    syn["w"] = rng.uniform(0.1, 0.9, n).astype(F32)
    kill = _kill_pattern(n)
    victim = n_nrn - 1  # no other record touches it
    by_dst, by_src = kill[::2], kill[1::2]
    syn["dst"][by_dst] = victim
    syn["src"][by_src] = victim
    with abnn_amd.Brain(256, 256, n_hidden, n, n, mode=mode, compact_every=2, w_prune=1e-6) as b:
        b.upload_synapses(syn)
        after, head = _edit(b, "kill", before=syn, src=(victim, 1), dst=(victim, 1), any=True)
        assert head["killed"] == len(kill)
        keep = np.setdiff1d(np.arange(n), kill)
        _same_records(after[keep], syn[keep], "a surviving neighbour")
        assert (after["src"][kill] == NONE).all() and (after["dst"][kill] == NONE).all()
        assert np.array_equal(after["w"][kill].view(np.uint32), syn["w"][kill].view(np.uint32))
        assert b.census(4, 0.0, 1.0)["tombstones"] == len(kill)


# ---- 4. / 5. edit then traverse equals upload then traverse ---------------------------------------
def _pair(n_syn, graph_seed=21, **kw):
    import abnn_amd

    out = []
    for _ in range(2):
        b = abnn_amd.Brain(256, 256, 3000, n_syn, n_syn, seed=13, **kw)
        b.build_random_graph(graph_seed)
        b.set_auto_stimulus(0, 256)
        out.append(b)
    return out


def _equal_after_passes(a, b, passes=12):
    a.encode_traversal(passes)
    b.encode_traversal(passes)
    assert a.n_syn() == b.n_syn() and a.structural_updates() == b.structural_updates()
    _same_records(a.download_synapses(), b.download_synapses(), "after the passes")
    assert np.array_equal(a.last_fired(), b.last_fired())
    assert a.scalars() == b.scalars() and a.stats() == b.stats()
    return a.stats()


@pytest.mark.parametrize("mode", [0, 1])
def test_edit_then_traverse_equals_upload_then_traverse(gpu, mode):
    from abnn_amd import edit

    a, b = _pair(120_000, mode=mode)
    syn = a.download_synapses()
    step1, h1 = edit.reference(syn, edit.config("kill", dst=(300, 40)), a.n_neuron())
    step2, h2 = edit.reference(step1, edit.config("affine", weights=(0.5, 0.7), a=0.5, b=0.25, clamp=(0.45, 0.58)),
                               a.n_neuron())
    assert h1["killed"] == 40 * 256 and h2["changed"] > 10_000
    assert a.edit("kill", dst=(300, 40)) == h1
    assert a.edit("affine", weights=(0.5, 0.7), a=0.5, b=0.25, clamp=(0.45, 0.58)) == h2
    b.upload_synapses(step2)
    _same_records(a.download_synapses(), step2)
    st = _equal_after_passes(a, b)
    assert st["fired"] > 0 and st["updated"] > 0
    a.close()
    b.close()


@pytest.mark.parametrize("where", ["a whole chunk in the tail", "below the tail only"])
def test_the_tally(gpu, where):
    from abnn_amd import edit

    n_syn = 120_000
    pair = _pair(n_syn, w_prune=0.105, p_new=0.35, w_init=0.5, compact_every=2, syn_capacity=n_syn + 20_000)
    syn = pair[0].download_synapses()
    victim = 3511
    syn["dst"][syn["dst"] == victim] = victim - 1
    if where == "a whole chunk in the tail":
        first = (n_syn // CHUNK - 1) * CHUNK
        syn["dst"][first:first + CHUNK] = victim
        syn["dst"][5_000:5_100] = victim
    else:
        syn["dst"][1_000:3_000] = victim
        syn["dst"][2 * CHUNK - 7:2 * CHUNK + 9] = victim
    for b in pair:
        b.upload_synapses(syn)
    a, b = pair
    want, head = edit.reference(syn, edit.config("kill", dst=(victim, 1)), a.n_neuron())
    assert a.edit("kill", dst=(victim, 1)) == head and head["killed"] >= 2_000
    assert a.n_syn() == n_syn  # until the next structural update
    b.upload_synapses(want)
    st = _equal_after_passes(a, b)
    assert a.structural_updates() == 6 and a.n_syn() != n_syn
    assert a.census(4, 0.0, 1.0)["tombstones"] == 0
    assert st["pruned"] == b.stats()["pruned"]  # the edit's kills are no pass statistic
    a.close()
    b.close()


# ---- 6. SCALE -------------------------------------------------------------------------------------
def test_scale_planes(gpu):
    n = 20_000
    syn = _records(n, 9)
    syn["w"][100:200] = 1.05
    rng = np.random.default_rng(3)
    with _brain(n) as b:
        b.upload_synapses(syn)
        for op, kw, m in (("scale_dst", dict(dst=(256, 256)), 256), ("scale_dst", dict(), 1000),
                          ("scale_src", dict(src=(100, 700)), 700), ("scale_src", dict(weights=(0.0, 2.0)), 1000),
                          ("scale_dst", dict(dst=(0, 1000), clamp=(-1.0, 1.0)), 1000)):
            plane = _plane(rng, m)
            plane[::7], plane[1::7], plane[2::7], plane[3::7] = 0.0, 1.0, np.nan, 3.4e38
            b.upload_synapses(syn)
            after, head = _edit(b, op, before=syn, plane=plane, **kw)
            assert head["nonfinite"] > 0 and head["changed"] < head["matched"]
            bits = after["w"].view(np.uint32)
            assert head["nonfinite"] <= int(((bits & 0x7F800000) == 0x7F800000).sum())


def _scaling_graph():
    """The small generated graph of the scaling tests: the recipe's shape (the
    dense input -> output block, w ~ U(0.4, 0.8); random hidden edges)."""
    from abnn_amd import graph

    return graph.recipe(256, 256, 488, 100_000, seed=7)


def scaling_bound_holds(before, after, factors, target, limits, n_nrn):
    """The issue's bound on every output neuron that is not left out; returns
    how many were left out."""
    from abnn_amd import degree

    cfg = degree.config((256, 256), ("in", "in_w"))
    old, new = degree.reference(before, cfg, n_nrn), degree.reference(after, cfg, n_nrn)
    assert old["in_skipped"] == 0 and new["in_skipped"] == 0
    old_sum, new_sum = old["in_w"] / 2.0**24, new["in_w"] / 2.0**24
    out = (factors <= F32(limits[0])) | (factors >= F32(limits[1])) | (old_sum <= 0)
    fan_in = old["in"].astype(np.float64)
    bound = target * 2.0**-22 + fan_in * 2.0**-24 * (1 + target / np.where(out, 1.0, old_sum))
    err = np.abs(new_sum - target)
    assert (err[~out] <= bound[~out]).all(), (err[~out].max(), bound[~out].min())
    return int(out.sum())


def test_scale_inputs(gpu):
    from abnn_amd import edit

    target, limits = 100.0, (0.5, 2.0)
    with _brain(100_000) as b:
        b.build_graph(_scaling_graph())
        before = b.download_synapses()
        in_w = b.degrees((256, 256), ("in_w",))["in_w"]
        got = b.scale_inputs(target, neurons=(256, 256), limits=limits)
        f = edit.factors(in_w, target, *limits)
        assert np.array_equal(got["factors"].view(np.uint32), f.view(np.uint32))
        want, head = edit.reference(before, edit.config("scale_dst", dst=(256, 256)), 1000, plane=f)
        after = b.download_synapses()
        _same_records(after, want)
        assert {k: got[k] for k in edit.KEYS} == head and head["matched"] == 65_536
        assert scaling_bound_holds(before, after, f, target, limits, 1000) <= 2  # 1 % of the 256 outputs
        # every neuron: the inputs have no input (factor 1), the hidden neurons' factors are clamped
        before = after
        in_w = b.degrees(None, ("in_w",))["in_w"]
        got = b.scale_inputs(1.0)
        f = edit.factors(in_w, 1.0, 0.5, 2.0)
        assert np.array_equal(got["factors"].view(np.uint32), f.view(np.uint32)) and (f[:256] == 1.0).all()
        want, head = edit.reference(before, edit.config("scale_dst"), 1000, plane=f)
        _same_records(b.download_synapses(), want)
        assert {k: got[k] for k in edit.KEYS} == head


# ---- 7. the enqueue-only path ---------------------------------------------------------------------
def test_enqueue_between_passes_on_a_side_stream(gpu):
    import torch

    import abnn_amd
    from abnn_amd import edit

    def make():
        b = abnn_amd.Brain(256, 256, 99_488, 1_000_000, 1_000_000)
        b.build_random_graph(1)
        b.set_auto_stimulus(0, 256)
        return b

    a, twin = make(), make()
    rng = np.random.default_rng(1)
    plane = _plane(rng, 256)
    jobs = [(edit.config("affine", weights=(0.15, INF), a=0.75, b=0.0625, clamp=(0.0, 0.7)), None),
            (edit.config("scale_dst", dst=(256, 256)), plane), (edit.config("kill", dst=(300, 8)), None),
            (edit.config("set", b=3.0, dst=(99_999, 1), weights=(50.0, 60.0)), None)]  # the last matches nothing
    outs = [torch.full((8,), SENTINEL, dtype=torch.int64, device="cuda:0") for _ in jobs]
    dplane = torch.from_numpy(plane).to("cuda:0")
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=0)
    a.encode_traversal(6, stream=side)
    for (cfg, pl), o in zip(jobs, outs):
        a.edit_enqueue(cfg, None if pl is None else dplane.data_ptr(), o.data_ptr(), stream=side)
    a.encode_traversal(2, stream=side)
    side.synchronize()  # the only synchronise
    twin.encode_traversal(6)
    syn = twin.download_synapses()
    for (cfg, pl), o in zip(jobs, outs):
        before = twin.checksum()
        want = np.zeros(8, dtype=np.uint64)
        abnn_amd._lib.call("abnn_edit", twin._h, C.byref(cfg), None if pl is None else pl.ctypes.data, 0 if pl is None else 256,
                           want.ctypes.data)
        assert o.cpu().numpy().view(np.uint64).tolist() == want.tolist()
        syn, head = edit.reference(syn, cfg, a.n_neuron(), plane=pl)
        assert edit.decode(want) == head
        assert (twin.checksum() == before) == (head["changed"] == 0)  # an edit that matches nothing writes nothing
    assert head["matched"] == 0
    _same_records(twin.download_synapses(), syn)
    twin.encode_traversal(2)
    assert a.checksum() == twin.checksum()
    assert np.array_equal(a.last_fired(), twin.last_fired()) and a.scalars() == twin.scalars()
    # the factors into a prefilled buffer
    words = np.array([0, -5, 1, 1 << 24, (1 << 53) + 1, 3 << 22, 1 << 40, 7 << 20], dtype=np.int64)
    dwords = torch.from_numpy(words).to("cuda:0")
    df = torch.full((len(words) + 2,), -7.0, dtype=torch.float32, device="cuda:0")
    a.edit_factors_enqueue(dwords.data_ptr(), len(words), 1.0, 0.5, 2.0, df.data_ptr(), stream=side)
    side.synchronize()
    got = df.cpu().numpy()
    assert np.array_equal(got[:-2].view(np.uint32), edit.factors(words, 1.0, 0.5, 2.0).view(np.uint32))
    assert (got[-2:] == -7.0).all()
    a.close()
    twin.close()


def test_factors_bit_exact(gpu):
    """The device's int64 -> fp32 conversion and division are correctly rounded:
    strength words over every magnitude against the numpy restatement."""
    import torch

    from abnn_amd import edit

    rng = np.random.default_rng(17)
    mag = rng.integers(0, 63, 200_001)
    words = (rng.integers(0, 1 << 62, 200_001) >> (62 - mag)) * rng.choice([1, 1, 1, -1], 200_001)
    words[:6] = [0, 1, -1, (1 << 53) + 1, (1 << 24) + 1, (1 << 62) + (1 << 38)]
    d = torch.from_numpy(words).to("cuda:0")
    out = torch.zeros(len(words), dtype=torch.float32, device="cuda:0")
    with _brain(10) as b:
        for target, lo, hi in ((1.0, 1e-30, 1e30), (153.6, 0.5, 2.0), (3e-5, 1e-38, 3e38)):
            b.edit_factors_enqueue(d.data_ptr(), len(words), target, lo, hi, out.data_ptr())
            torch.cuda.synchronize()
            want = edit.factors(words, target, lo, hi)
            got = out.cpu().numpy()
            bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
            assert bad.size == 0, (target, bad[:5], words[bad[:5]], got[bad[:5]], want[bad[:5]])


# ---- 8. capacity headroom and invalid handles -------------------------------------------------------
def test_headroom_is_not_edited(gpu):
    import abnn_amd

    n_syn = 120_000
    with abnn_amd.Brain(256, 256, 3000, n_syn, n_syn, syn_capacity=n_syn + 30_000, seed=13, p_new=1.0, w_init=0.5,
                        compact_every=2) as b:
        b.build_random_graph(21)
        b.set_auto_stimulus(0, 256)
        head = b.edit("set", b=0.625)
        assert head["matched"] == head["records"] == n_syn
        assert (b.download_synapses()["w"] == F32(0.625)).all()
        for _ in range(8):  # until a structural update appends grown records: they are not yet visited
            b.encode_traversal(2)
            if b.n_syn() != n_syn:
                break
        assert b.n_syn() > n_syn and b.stats()["grown"] == b.n_syn() - n_syn
        grown = b.download_synapses(n_syn)
        assert (grown["w"] == F32(0.5)).all()
        assert b.edit("set", b=0.25)["matched"] == b.n_syn()


def test_refusals(gpu):
    import torch

    import abnn_amd
    from abnn_amd import edit

    out = torch.zeros(8, dtype=torch.int64, device="cuda:0")
    plane = torch.ones(1000, dtype=torch.float32, device="cuda:0")
    with _brain(1_000) as b:
        b.build_random_graph(1)
        before = b.checksum()
        for cfg, pl in ((edit.config("set", src=(900, 101)), None), (edit.config("kill", dst=(1000, 1)), None),
                        (edit.config("scale_dst"), None), (edit.config("set", b=1.0), plane.data_ptr()),
                        (edit.config("scale_src", src=(0, 10), any=True), plane.data_ptr()),
                        (edit.config("kill", clamp=(0.0, 1.0)), None)):
            with pytest.raises(abnn_amd.AbnnError) as err:
                b.edit_enqueue(cfg, pl, out.data_ptr())
            assert err.value.status == 1
        for kw in (dict(op="scale_dst", plane=np.ones(999, dtype=F32)), dict(op="scale_dst", dst=(0, 10), plane=np.ones(11, dtype=F32)),
                   dict(op="set", plane=np.ones(1000, dtype=F32)), dict(op="scale_dst")):
            with pytest.raises(abnn_amd.AbnnError) as err:
                b.edit(**kw)
            assert err.value.status == 1, kw
        with pytest.raises(abnn_amd.AbnnError):
            b.edit_factors_enqueue(out.data_ptr(), 4, -1.0, 0.5, 2.0, plane.data_ptr())
        torch.cuda.synchronize()
        assert not out.cpu().numpy().any() and b.checksum() == before  # a refused edit writes nothing


# ---- 9. shards ------------------------------------------------------------------------------------
def test_three_shards_equal_the_unsharded_edit(gpu):
    import abnn_amd
    from abnn_amd import edit
    from abnn_amd.shard import global_events, shard_ranges

    n_syn, events = 10_000, 100_000
    rng = np.random.default_rng(4)
    with _brain(n_syn) as whole:
        whole.build_random_graph(1)
        syn = whole.download_synapses()
        ge = global_events(n_syn, events, 3)
        for op, kw, plane in (("draw", dict(a=0.1, b=0.3, seed=99, src=(0, 700)), None), ("kill", dict(dst=(256, 100)), None),
                              ("scale_dst", dict(), _plane(rng, 1000))):
            whole.upload_synapses(syn)
            want, head = _edit(whole, op, before=syn, plane=plane, **kw)
            parts, heads = [], []
            for lo, hi in shard_ranges(n_syn, 3):
                with abnn_amd.Brain(256, 256, 488, hi - lo, events, syn_offset=lo, global_events=ge) as s:
                    s.upload_synapses(syn[lo:hi])
                    after, h = _edit(s, op, before=syn[lo:hi], plane=plane, **kw)
                    parts.append(after)
                    heads.append(h)
            _same_records(np.concatenate(parts), want, op)
            assert edit.merge(heads) == head and head["changed"] > 0


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_sharded_brain_edit_world1(gpu, monkeypatch):
    import torch.distributed as dist

    from abnn_amd import edit
    from abnn_amd.shard import ShardedBrain, TorchComm

    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(_port()))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        sb = ShardedBrain(TorchComm(), 256, 256, 488, 100_000, 100_000, device=0, native=True)
        sb.build_graph(_scaling_graph())
        syn = sb.brain.download_synapses()
        for op, kw in (("affine", dict(a=0.5, b=0.125, dst=(256, 256))), ("draw", dict(a=0.0, b=1.0, seed=5, src=(512, 100))),
                       ("kill", dict(src=(600, 50), dst=(600, 50), any=True))):
            syn, head = edit.reference(syn, edit.config(op, **kw), 1000)
            assert sb.edit(op, **kw) == head
            _same_records(sb.brain.download_synapses(), syn, op)
        in_w = sb.degrees((256, 256), ("in_w",))["in_w"]
        got = sb.scale_inputs(50.0, neurons=(256, 256))
        f = edit.factors(in_w, 50.0, 0.5, 2.0)
        syn, head = edit.reference(syn, edit.config("scale_dst", dst=(256, 256)), 1000, plane=f)
        assert np.array_equal(got["factors"].view(np.uint32), f.view(np.uint32))
        assert {k: got[k] for k in edit.KEYS} == head
        _same_records(sb.brain.download_synapses(), syn, "scale_inputs")
        sb.native.close()
        sb.brain.close()
    finally:
        dist.destroy_process_group()


# ---- 10. the C++ mirror ---------------------------------------------------------------------------
def test_cpp_edit(gpu):
    from abnn_amd.build import build_edit_test

    prog = build_edit_test()
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    lines = r.stdout.strip().splitlines()
    assert lines, (r.returncode, r.stderr[-2000:])
    res = json.loads(lines[-1])
    assert r.returncode == 0 and res["ok"], (res, r.stderr[-2000:])
    assert res["records"] == 100_001 and res["killed"] == 65_536 and res["cases"] >= 6


if __name__ == "__main__" and sys.argv[1:] == ["big"]:  # test_big_brain's child: ABNN_EDIT_BLOCKS is set
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import abnn_amd

    with abnn_amd.Brain(256, 256, 100_000, BIG, 100_000) as brain:
        brain.upload_synapses(_big_records())
        child_heads, child_syn = _run_big(brain)
    print(json.dumps({"heads": child_heads, "sha256": hashlib.sha256(child_syn.tobytes()).hexdigest()}))
