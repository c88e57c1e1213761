"""GPU parity at neuron ids above 2^18, in seconds (tests/high_id_helpers.py).

Below 2^18 neurons the pre-spike filter's word hash is the identity (t = 0):
no two bitmap words fold onto one block, the high image is not rotated and
code_src decodes jh = 0.  Every comparison here runs the crafted graph, whose
probes are recent and whose decoys alias in every id class n >> 18 (all 64 at
N_NRN = 2^24 - 2; tests/test_high_id_model.py asserts that on the oracle), and
is bit-exact against the CPU oracle or a numpy reference: records as u32,
lastFired, clock, rBar as fp32, the statistics, the exact recent bitmap."""
import functools

import numpy as np
import pytest

import high_id_helpers as H
from shard_helpers import GpuShards

pytestmark = pytest.mark.gpu

N_NRN = 2**24 - 2  # the most abnn_create admits
SP = dict(w_prune=0.105, p_new=0.35, w_init=0.5, compact_every=2)  # tests/test_gpu_plasticity.py


def _pair(n_nrn, syn, events=None, syn_offset=0, global_events=0, syn_capacity=0, oracle=True, **params):
    import abnn_amd
    from oracle import oracle as O

    events = len(syn) if events is None else events
    g = abnn_amd.Brain(256, 256, n_nrn - 512, len(syn), events, syn_offset=syn_offset,
                       global_events=global_events, syn_capacity=syn_capacity, **params)
    g.upload_synapses(syn)
    g.set_auto_stimulus(0, 256)
    if not oracle:
        return g, None
    o = O.OracleBrain(256, 256, n_nrn - 512, len(syn), events, syn_offset=syn_offset,
                      global_events=global_events, syn_capacity=syn_capacity, **params)
    o.set_synapses(syn)
    o.set_auto_stimulus(0, 256)
    return g, o


def _assert_same(g, o, what=""):
    """test_gpu_parity._assert_same, plus the record count, the pass index and
    the statistics; returns the downloaded lastFired."""
    assert g.n_syn() == int(o.s.dims.n_syn), f"n_syn {what}"
    assert np.array_equal(g.download_synapses().view(np.uint32), o.syn.view(np.uint32)), f"synapses differ {what}"
    lf = g.last_fired()
    assert np.array_equal(lf, o.last_fired), f"lastFired differs {what}"
    sg, so = g.scalars(), o.scalars()
    assert sg["clock"] == so["clock"] and sg["pass_index"] == so["pass_index"], what
    assert np.float32(sg["rbar"]) == np.float32(so["rbar"]), what
    assert g.stats() == o.stats(), what
    return lf


def _every_pass(g, o, passes=12, reward_at=8, visits=False, what=""):
    """Every pass: the state against the oracle, and the pass's exact bitmap
    against the one recomputed from the pass-start lastFired."""
    lf = g.last_fired()
    for k in range(passes):
        if k == reward_at:
            g.set_reward(0.5)
            o.set_reward(0.5)
        now = g.scalars()["clock"]
        lf[:256] = now  # the stimulus is stamped at pass start
        g.encode_traversal(1)
        o.pass_threaded(nthreads=16)
        bm, _ = H._bitmap(g)
        assert np.array_equal(bm, H._expected_bitmap(lf, now, bm.size)), f"bitmap, {what} pass {k}"
        lf = _assert_same(g, o, f"{what} pass {k}")
        if visits:
            assert np.array_equal(g.last_visited(), o.last_visited), f"lastVisited, {what} pass {k}"
    assert o.stats()["fired"] > 0 and o.stats()["updated"] > o.stats()["fired"]


# ---- the sweep, every pass ---------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"ABNN_FUSED": "0"}, {"ABNN_LEAN": "0"}, {"ABNN_SPEC": "2"}],
                         ids=["fused", "two-kernel", "full-instance", "spec-everywhere"])
@pytest.mark.parametrize("over", [{}, dict(max_spikes=200_000), dict(track_visits=1)],
                         ids=["default", "budget-huge", "visits"])
def test_sweep_every_pass(gpu, monkeypatch, env, over):
    """All 64 id classes: with the huge budget every pre-gated record far into
    the array updates; with the default one the cut falls early and the
    statistics see the later records."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g, o = _pair(N_NRN, H.high_id_graph(N_NRN), **over)
    _every_pass(g, o, visits=bool(over.get("track_visits")), what=f"{env} {over}")


@pytest.mark.parametrize("n_nrn", [2**18 + 70, 2**23 + 70])
def test_sweep_at_the_first_fold_and_the_first_x_bit(gpu, n_nrn):
    """The first sizes at which t != 0 (one class of 70 ids folds onto class
    0's blocks) and at which x = 1, almost every id below the boundary."""
    g, o = _pair(n_nrn, H.high_id_graph(n_nrn))
    _every_pass(g, o, what=f"{n_nrn} neurons")


# ---- both bitmap builders ----------------------------------------------------------------------
def test_both_bitmap_builders_with_host_writes_at_high_ids(gpu):
    """test_recent_bitmap_update_with_host_writes at high ids: the spike-list
    build (k_apply) before and well after the host writes, k_bitmap after
    them; set_timestamps on one probe per class, set_last_fired over a window
    across 2^23 and one that ends at N_NRN (recent stamps and stamps ahead of
    the clock)."""
    parts = H.high_id_parts(N_NRN)
    probes = parts["probes"]
    _, first = np.unique(probes >> H.CLASS_LOG2, return_index=True)
    one_per_class = probes[first + 3]  # (not the class's first id: a random one)
    assert np.unique(one_per_class >> H.CLASS_LOG2).size == 64
    g, o = _pair(N_NRN, H.high_id_graph(N_NRN))
    modes = []
    lf = g.last_fired()
    for k in range(24):
        now = g.scalars()["clock"]
        if k == 7:
            g.set_timestamps(one_per_class, now)
            o.set_timestamps(one_per_class, now)
            lf[one_per_class] = now
        if k == 12:
            for at in (2**23 - 500, N_NRN - 1000):
                v = np.full(1000, now - 2, np.uint64)
                v[::7] = now + 3  # not recent until the clock gets there
                g.set_last_fired(v, at)
                o.last_fired[at:at + 1000] = v
                lf[at:at + 1000] = v
        lf[:256] = now
        g.encode_traversal(1)
        o.pass_threaded(nthreads=16)
        bm, inc_next = H._bitmap(g)
        modes.append(inc_next)
        assert np.array_equal(bm, H._expected_bitmap(lf, now, bm.size)), f"bitmap, pass {k}"
        lf = _assert_same(g, o, f"pass {k}")
    # capi.hip build_next_ok: W - 1 = 4 passes of spike lists since the write, and
    # the clock at the largest written stamp + W or later -- 7 + 5 for the first
    # write (the second comes at 12), (12 + 3) + 5 = 20 for the second
    assert all(modes[5:7]) and all(modes[20:]), modes  # built by k_apply before and after the writes
    assert not any(modes[7:12]) and not any(modes[12:20]), modes


# ---- virtual shards ----------------------------------------------------------------------------
SHARD_PASSES = 10


@functools.lru_cache(maxsize=1)
def _unsharded():
    """The unsharded fused run (equal to the oracle), shared by the shard cases."""
    g, o = _pair(N_NRN, H.high_id_graph(N_NRN))
    for k in range(SHARD_PASSES):
        if k == 6:
            g.set_reward(0.125)
            o.set_reward(0.125)
        g.encode_traversal(1)
        o.pass_threaded(nthreads=16)
    lf = _assert_same(g, o, "unsharded")
    return g.download_synapses().view(np.uint32), lf, g.scalars()


@pytest.mark.parametrize("fused", ["1", "0"], ids=["fused-shard-pass", "two-kernel-shard-pass"])
@pytest.mark.parametrize("world", [2, 3])
def test_virtual_shards(gpu, monkeypatch, world, fused):
    import torch

    from abnn_amd.shard import global_events, shard_ranges

    want_syn, want_lf, want_scalars = _unsharded()
    monkeypatch.setenv("ABNN_FUSED", fused)
    syn = H.high_id_graph(N_NRN)
    ge = global_events(len(syn), len(syn), world)
    shards = [_pair(N_NRN, syn[lo:hi], events=len(syn), syn_offset=lo, global_events=ge, oracle=False)[0]
              for lo, hi in shard_ranges(len(syn), world)]
    gs = GpuShards(shards)
    for k in range(SHARD_PASSES):
        if k == 6:
            for b in shards:
                b.set_reward(0.125)
        gs.pass_()
    torch.cuda.synchronize()
    got = np.concatenate([b.download_synapses() for b in shards])
    assert np.array_equal(got.view(np.uint32), want_syn)
    for b in shards:
        assert np.array_equal(b.last_fired(), want_lf)
        assert b.scalars() == want_scalars


# ---- random mode -------------------------------------------------------------------------------
def test_random_mode_every_pass(gpu):
    """The src32 mirror and the hashed-filter instance of the gate."""
    syn = H.high_id_graph(N_NRN)[:300_000]
    assert (syn["src"] >= 2**23).sum() > 1000
    g, o = _pair(N_NRN, syn, events=250_000, mode=1, seed=9)
    for k in range(10):
        g.encode_traversal(1)
        o.pass_threaded(nthreads=16)
        _assert_same(g, o, f"pass {k}")
    assert g.visited_events() == 250_000
    assert o.stats()["fired"] > 0 and o.stats()["updated"] > o.stats()["fired"]


# ---- plasticity --------------------------------------------------------------------------------
def test_plasticity_every_pass(gpu):
    """Pruning, growth (set_src of records whose src is a high id) and the
    structural update, every pass, the record count included."""
    syn = H.high_id_graph(N_NRN)
    g, o = _pair(N_NRN, syn, syn_capacity=len(syn) + 50_000, seed=13, **SP)
    grown, sizes = [], set()
    for k in range(8):
        if k == 6:
            g.set_reward(0.4)
            o.set_reward(0.4)
        before = o.stats()["grown"]
        g.encode_traversal(1)
        o.pass_threaded(nthreads=16)
        _assert_same(g, o, f"pass {k}")
        new = o.stats()["grown"] - before
        if new:  # a structural update appends the grown records
            grown.append(o.syn[len(o.syn) - new:].copy())
        sizes.add(g.n_syn())
    assert g.structural_updates() >= 2 and len(sizes) > 1
    st = o.stats()
    assert st["grown"] > 0 and st["pruned"] > 0
    grown = np.concatenate(grown)
    assert (grown["w"] == np.float32(SP["w_init"])).all()
    assert (grown["src"] >= 2**23).any() and (grown["dst"] >= 2**23).any()
    assert ((grown["src"] >= 2**18) & (grown["src"] < 2**23)).any()


# ---- round trips -------------------------------------------------------------------------------
def test_round_trips_of_every_fixed_id(gpu, tmp_path):
    import abnn_amd
    from abnn_amd import SYN_DTYPE

    ids = H.fixed_ids(N_NRN)
    assert {2**18 - 1, 2**18, 2**23 - 1, 2**23, N_NRN - 1, 63 << 18} <= set(ids.tolist())
    n = 2 * len(ids)
    syn = np.zeros(n, dtype=SYN_DTYPE)
    syn["src"][0::2] = ids
    syn["dst"][0::2] = ids[::-1]
    syn["src"][1::2] = syn["dst"][1::2] = 0xFFFFFFFF  # tombstones between them
    syn["src"][1:n:10], syn["dst"][1:n:10] = N_NRN - 1, 2**23  # ... and not everywhere
    syn["w"] = np.linspace(0.05, 0.95, n, dtype=np.float32)
    want = syn.view(np.uint32)

    def fresh():
        return abnn_amd.Brain(256, 256, N_NRN - 512, n, n)

    g = fresh()
    g.upload_synapses(syn)
    assert np.array_equal(g.download_synapses().view(np.uint32), want), "upload -> download"
    g.set_timestamps(ids, 7)
    g.save_flat(tmp_path / "m.flat")
    h = fresh()
    h.load_flat(tmp_path / "m.flat")
    assert np.array_equal(h.download_synapses().view(np.uint32), want), "save_flat -> load_flat"
    assert np.array_equal(h.last_fired(), g.last_fired())
    assert np.array_equal(np.flatnonzero(h.last_fired()), ids)
    g.save(tmp_path / "m.bnn")
    h2 = fresh()
    h2.load(tmp_path / "m.bnn")
    assert np.array_equal(h2.download_synapses().view(np.uint32), want), "save -> load"


# ---- census, degree, select --------------------------------------------------------------------
RANGES = ((2**18 - 5, 10), (2**23 - 100, 200), (N_NRN - 1000, 1000), (3 * 2**18 - 7, 2**19 + 14))


@pytest.fixture(scope="module")
def crafted(gpu):
    """The crafted graph on a handle after six passes (weights moved), and its download."""
    g, o = _pair(N_NRN, H.high_id_graph(N_NRN), max_spikes=200_000)
    g.encode_traversal(6)
    o.pass_threaded(6, nthreads=16)
    _assert_same(g, o)
    return g, g.download_synapses()


@pytest.mark.parametrize("r", RANGES)
def test_census_of_high_src_ranges(gpu, crafted, r):
    from abnn_amd import census

    g, syn = crafted
    for kw in (dict(src=r), dict(src=r, dst=(256, N_NRN - 256)), dict(dst=r)):
        cfg = census.config(64, 0.0, 1.0, **kw)
        want = census.reference(syn, cfg)
        assert want["selected"] > 0, kw
        got = g.census(64, 0.0, 1.0, **kw)
        assert np.array_equal(census.to_words(got), census.to_words(want)), kw


@pytest.mark.parametrize("r", RANGES + ((2**23 - 3000, 6000),), ids=lambda r: f"{r[0]}+{r[1]}")
def test_degrees_of_high_id_windows(gpu, crafted, r):
    """(6000 neurons across 2^23: more than the LDS planes hold, the atomics path.)"""
    from abnn_amd import degree

    g, syn = crafted
    what = ("out", "out_w", "in", "in_w")
    want = degree.reference(syn, degree.config(r, what), N_NRN)
    assert want["out_total"] > 0 and want["in_total"] > 0
    got = g.degrees(r, what)
    assert np.array_equal(degree.to_words(got), degree.to_words(want))


@pytest.mark.parametrize("i", range(len(RANGES)))
def test_select_of_high_id_ranges(gpu, crafted, i):
    from abnn_amd import select

    g, syn = crafted
    src, dst = RANGES[i], RANGES[(i + 1) % len(RANGES)]
    for kw in (dict(src=src), dict(src=src, dst=dst, any=True)):
        cfg = select.config(**kw)
        matched = int(select.matches(syn, cfg).sum())
        assert matched > 0, kw
        want = select.reference(syn, cfg, matched, N_NRN)
        got = g.select(**kw)
        assert got["matched"] == matched and got["written"] == matched, kw
        assert np.array_equal(got["index"], want["index"]), kw
        assert np.array_equal(got["syn"].view(np.uint32), want["syn"].view(np.uint32)), kw
        assert np.array_equal(select.to_words(got), select.to_words(want)), kw
