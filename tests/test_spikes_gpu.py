"""The spike recorder on the GPU (abnn.h abnn_spikes_*, csrc/spikes.hip).

The reference is the CPU oracle, never the library: one oracle pass run as
shard_gate -> shard_apply -> shard_commit at world 1 leaves the pass's spike
list in its exchange record (tests/spikes_helpers.py; tests/test_spikes_abi.py
checks what makes that list the reference).  Every word the recorder holds --
info, pass entries, raster, counts -- is compared against
abnn_amd.spikes.reference over those lists."""
import ctypes as C
import json
import subprocess

import numpy as np
import pytest

from shard_helpers import GpuShards
from spikes_helpers import SHAPE1, SHAPE1_LENGTHS, make_oracle, oracle_lists

pytestmark = pytest.mark.gpu

U32 = np.uint32
N1 = 256 + 256 + SHAPE1[0]


def _gpu(n_hidden, n_syn, events, seed=1, **params):
    import abnn_amd

    g = abnn_amd.Brain(256, 256, n_hidden, n_syn, events, **params)
    g.build_random_graph(seed)
    g.set_auto_stimulus(0, 256)
    return g


def _same(got, want, counts=None, what=""):
    """got: Brain.spikes(); want: spikes.reference(...); counts: Brain.spike_counts()."""
    assert got["info"] == want["info"], what
    assert got["passes"].dtype == want["passes"].dtype
    assert np.array_equal(got["passes"], want["passes"]), (what, got["passes"], want["passes"])
    assert got["raster"].dtype == U32 and np.array_equal(got["raster"], want["raster"]), what
    if want["counts"] is not None:
        assert counts is not None and counts.dtype == U32 and np.array_equal(counts, want["counts"]), what


def _same_state(g, o, what=""):
    assert np.array_equal(g.download_synapses().view(U32), o.syn.view(U32)), what
    assert np.array_equal(g.last_fired(), o.last_fired), what
    sg, so = g.scalars(), o.scalars()
    assert sg["clock"] == so["clock"] and sg["pass_index"] == so["pass_index"], what
    assert np.float32(sg["rbar"]) == np.float32(so["rbar"]), what
    assert g.stats() == o.stats(), what


@pytest.fixture(scope="module")
def shape1():
    """The oracle's 16 lists at the first shape, computed once; read only."""
    o = make_oracle(*SHAPE1)
    lists, meta = oracle_lists(o, 16)
    assert [len(x) for x in lists] == SHAPE1_LENGTHS
    for x in lists:
        x.setflags(write=False)
    return lists, meta, o


# ---- 1. every pass path ------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"ABNN_FUSED": "0"}, {"ABNN_LEAN": "0"}], ids=["default", "two-kernel", "full-instance"])
def test_every_pass_path(gpu, monkeypatch, shape1, env):
    from abnn_amd import spikes

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    lists, meta, o = shape1
    with _gpu(*SHAPE1) as g:
        g.record_spikes(raster=1 << 16, passes=32, counts=True)
        g.encode_traversal(16)
        got = g.spikes()
        want = spikes.reference(lists, meta, spikes.config(1 << 16, 32, counts=True), n_neuron=N1)
        _same(got, want, g.spike_counts(), str(env))
        assert got["passes"]["count"].tolist() == SHAPE1_LENGTHS
        assert [len(s) for s in spikes.split(got["passes"], got["raster"])] == SHAPE1_LENGTHS
        hidden = got["raster"] >= 512
        assert hidden.any() and not hidden.all()  # both neuron classes
        _same_state(g, o, str(env))  # the recorder perturbs nothing
        assert got["info"]["selected_seen"] == g.stats()["fired"]


def test_fused_shape(gpu):
    """test_pass_variants' own shape, known to take the fused launch."""
    from abnn_amd import spikes

    shape = (99_488, 1_000_000, 1_000_000)
    o = make_oracle(*shape)
    lists, meta = oracle_lists(o, 10)
    assert [len(x) for x in lists] == [0, 0, 0, 2560, 2560, 2560, 2560, 727, 627, 2560]
    with _gpu(*shape) as g:
        g.record_spikes(raster=1 << 15, passes=10, counts=True)
        g.encode_traversal(10)
        got = g.spikes()
        _same(got, spikes.reference(lists, meta, spikes.config(1 << 15, 10, counts=True), n_neuron=g.n_neuron()),
              g.spike_counts())
        _same_state(g, o)
        assert got["info"]["selected_seen"] == g.stats()["fired"] and got["info"]["passes_dropped"] == 0


# ---- 2. small and zero budgets -----------------------------------------------------------------
def test_small_and_zero_budgets(gpu):
    from abnn_amd import spikes

    shape = (488, 10_000, 100_000)
    for budget, passes in ((37, 24), (0, 6)):
        o = make_oracle(*shape, max_spikes=budget)
        lists, meta = oracle_lists(o, passes)
        if budget:
            assert [len(x) for x in lists] == [0, 0, 0] + [37] * (passes - 3)
        with _gpu(*shape, max_spikes=budget) as g:
            g.record_spikes(raster=1000, passes=passes, counts=True)
            g.encode_traversal(passes)
            got = g.spikes()
            _same(got, spikes.reference(lists, meta, spikes.config(1000, passes, counts=True), n_neuron=N1),
                  g.spike_counts(), f"budget {budget}")
            assert got["info"]["passes_recorded"] == passes
            if not budget:
                assert got["passes"]["count"].tolist() == [0] * 6 and got["raster"].size == 0
            _same_state(g, o, f"budget {budget}")


# ---- 3. long lists and ordered selection ---------------------------------------------------------
@pytest.fixture(scope="module")
def long_lists():
    o = make_oracle(*SHAPE1, max_spikes=200_000)
    lists, meta = oracle_lists(o, 8)
    assert len(lists[3]) == 20_320 and len(lists[6]) == 9588
    assert int((lists[3] < 512).sum()) == 19_688 and int((lists[3] >= 512).sum()) == 632
    for x in lists:
        x.setflags(write=False)
    return lists, meta


@pytest.mark.parametrize("neurons", [(256, 256), (512, 488), (300, 7), (0, 256), None],
                         ids=["outputs", "hidden", "seven", "inputs-nothing", "off"])
def test_long_lists_and_ordered_selection(gpu, long_lists, neurons):
    from abnn_amd import spikes

    lists, meta = long_lists
    with _gpu(*SHAPE1, max_spikes=200_000) as g:
        g.record_spikes(raster=100_000, passes=8, neurons=neurons, counts=True)
        g.encode_traversal(8)
        got = g.spikes()
        want = spikes.reference(lists, meta, spikes.config(100_000, 8, neurons, counts=True), n_neuron=N1)
        assert want["info"]["passes_dropped"] == 0
        counts = g.spike_counts()
        _same(got, want, counts, str(neurons))
        first, n = neurons if neurons else (0, N1)
        assert np.array_equal(counts, np.bincount(want["raster"] - U32(first), minlength=n).astype(U32))
        if neurons == (0, 256):
            assert got["info"]["selected_seen"] == 0 and got["info"]["spikes_seen"] > 30_000
        if neurons == (512, 488):  # the 632 hidden spikes scattered among pass 3's 19 688 output spikes, in order
            assert got["passes"]["count"][3] == 632
            assert np.array_equal(spikes.split(got["passes"], got["raster"])[3], lists[3][lists[3] >= 512])


# ---- 4. capacity -----------------------------------------------------------------------------------
def _read(g, name, first, n, dtype):
    from abnn_amd._lib import call

    out = np.zeros(max(n, 1), dtype=dtype)
    call(name, g._h, first, n, out.ctypes.data)
    return out[:n]


@pytest.mark.parametrize("raster,passes,recorded", [(3207, 32, 5), (3000, 32, 4), (1 << 16, 2, 2), (0, 32, 16)],
                         ids=["exact-fit", "sticky", "pass-table", "no-raster"])
def test_capacity(gpu, shape1, raster, passes, recorded):
    import abnn_amd
    from abnn_amd import spikes

    lists, meta, _ = shape1
    with _gpu(*SHAPE1) as g:
        g.record_spikes(raster=raster, passes=passes, counts=True)
        g.encode_traversal(16)
        got = g.spikes()
        want = spikes.reference(lists, meta, spikes.config(raster, passes, counts=True), n_neuron=N1)
        _same(got, want, g.spike_counts(), f"{raster} {passes}")
        info = got["info"]
        assert info["passes_recorded"] == recorded and info["passes_dropped"] == 16 - recorded
        assert info["passes_seen"] == 16 and info["spikes_seen"] == info["selected_seen"] == sum(SHAPE1_LENGTHS)
        assert info["spikes_recorded"] == sum(SHAPE1_LENGTHS[:recorded])
        assert info["spikes_dropped"] == sum(SHAPE1_LENGTHS[recorded:])
        assert got["passes"]["pass_index"].tolist() == list(range(recorded))  # the first K consecutive passes
        assert int(g.spike_counts().sum()) == sum(SHAPE1_LENGTHS)  # the counts go on over dropped passes
        # reads past the recorded end are refused
        held = info["spikes_recorded"] if raster else 0
        assert np.array_equal(_read(g, "abnn_spikes_read_raster", 0, held, U32), got["raster"])
        if recorded > 1:
            assert np.array_equal(_read(g, "abnn_spikes_read_passes", 1, recorded - 1, spikes.SPIKE_PASS_DTYPE),
                                  got["passes"][1:])
        for name, first, n, dt in (("abnn_spikes_read_passes", 0, recorded + 1, spikes.SPIKE_PASS_DTYPE),
                                   ("abnn_spikes_read_passes", recorded + 1, 0, spikes.SPIKE_PASS_DTYPE),
                                   ("abnn_spikes_read_raster", 0, held + 1, U32),
                                   ("abnn_spikes_read_raster", held, 1, U32)):
            with pytest.raises(abnn_amd.AbnnError) as err:
                _read(g, name, first, n, dt)
            assert err.value.status == 1, (name, first, n)


def test_clear_resumes_recording(gpu, shape1):
    from abnn_amd import spikes

    lists, meta, _ = shape1
    cfg = spikes.config(3000, 32, counts=True)
    with _gpu(*SHAPE1) as g:
        g.record_spikes(raster=3000, passes=32, counts=True)
        g.encode_traversal(8)
        _same(g.spikes(), spikes.reference(lists[:8], meta[:8], cfg, n_neuron=N1), g.spike_counts(), "before")
        assert g.spikes()["info"]["passes_dropped"] == 4
        g.clear_spikes(keep_counts=True)
        _same(g.spikes(), spikes.reference(lists[:8], meta[:8], cfg, n_neuron=N1, clears={8: True}), g.spike_counts())
        g.encode_traversal(4)
        got = g.spikes()
        _same(got, spikes.reference(lists[:12], meta[:12], cfg, n_neuron=N1, clears={8: True}), g.spike_counts(), "kept")
        assert got["passes"]["pass_index"].tolist() == [8, 9, 10, 11] and got["passes"]["offset"][0] == 0
        assert int(g.spike_counts().sum()) == sum(SHAPE1_LENGTHS[:12])
        g.clear_spikes()
        g.encode_traversal(4)
        got = g.spikes()
        _same(got, spikes.reference(lists, meta, cfg, n_neuron=N1, clears={8: True, 12: False}), g.spike_counts(), "zeroed")
        assert got["passes"]["pass_index"].tolist() == [12, 13, 14] and got["info"]["passes_seen"] == 16
        assert int(g.spike_counts().sum()) == sum(SHAPE1_LENGTHS[12:])


# ---- 5. renormalisation ------------------------------------------------------------------------------
def test_renormalisation(gpu):
    from abnn_amd import spikes

    o = make_oracle(*SHAPE1, renorm_thresh=5)
    lists, meta = oracle_lists(o, 12)
    with _gpu(*SHAPE1, renorm_thresh=5) as g:
        g.record_spikes(raster=1 << 16, passes=12)
        g.encode_traversal(12)
        got = g.spikes()
        _same(got, spikes.reference(lists, meta, spikes.config(1 << 16, 12)))
        assert got["passes"]["now"].tolist() == [0, 1, 2, 3, 4, 5, 6, 0, 1, 2, 3, 4]
        assert got["passes"]["epoch"].tolist() == [0] * 7 + [1] * 5
        assert got["passes"]["pass_index"].tolist() == list(range(12))
        _same_state(g, o)


# ---- 6. random mode ------------------------------------------------------------------------------------
def test_random_mode(gpu):
    from abnn_amd import spikes

    o = make_oracle(*SHAPE1, mode=1)
    lists, meta = oracle_lists(o, 8)
    assert [len(x) for x in lists] == [0, 0, 0, 2560, 533, 95, 2560, 330]
    with _gpu(*SHAPE1, mode=1) as g:
        g.record_spikes(raster=1 << 14, passes=8, neurons=(512, 488), counts=True)
        g.encode_traversal(8)
        _same(g.spikes(), spikes.reference(lists, meta, spikes.config(1 << 14, 8, (512, 488), counts=True)),
              g.spike_counts())
        g.record_spikes(raster=1 << 14, passes=8)  # a restart on a running handle, no range
        g.encode_traversal(1)
        more, m2 = oracle_lists(o, 1)
        _same(g.spikes(), spikes.reference(more, m2, spikes.config(1 << 14, 8)))
        _same_state(g, o)


# ---- 7. a side stream, and batches -----------------------------------------------------------------------
def test_side_stream_and_batches(gpu, shape1):
    import torch

    import abnn_amd
    from abnn_amd import spikes

    lists, meta, o = shape1
    want = spikes.reference(lists, meta, spikes.config(1 << 16, 16, (256, 256), counts=True))
    with _gpu(*SHAPE1) as g:
        g.record_spikes(raster=1 << 16, passes=16, neurons=(256, 256), counts=True)
        side = torch.cuda.Stream(device=0)
        g.encode_traversal(5, stream=side)
        g.encode_traversal(11, stream=side)
        side.synchronize()
        _same(g.spikes(), want, g.spike_counts(), "side stream")
        _same_state(g, o)
        g.stop_spikes()
        with pytest.raises(abnn_amd.AbnnError):
            g.spikes()
        g.record_spikes(raster=1 << 16, passes=16, counts=True)  # a fresh start begins empty
        got = g.spikes()
        assert set(got["info"].values()) == {0} and got["passes"].size == 0 and got["raster"].size == 0
        assert not g.spike_counts().any()


# ---- 8. sharded ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,shape", [(2, SHAPE1), (3, SHAPE1), (2, (99_488, 1_000_000, 1_000_000))],
                         ids=["world2", "world3", "world2-fused-shape"])
def test_sharded(gpu, world, shape):
    """Every rank's recorder equals the unsharded brain's recorder on the same
    graph (test_every_pass_path / test_fused_shape pin that one to the oracle)."""
    import torch

    import abnn_amd
    from abnn_amd.shard import global_events, shard_ranges

    n_hidden, n_syn, events = shape
    passes, kw = 10, dict(raster=1 << 15, passes=10, neurons=(256, 744), counts=True)
    ge = global_events(n_syn, events, world)
    shards = []
    for lo, hi in shard_ranges(n_syn, world):
        b = abnn_amd.Brain(256, 256, n_hidden, hi - lo, events, syn_offset=lo, global_events=ge)
        b.build_random_graph(1)
        b.set_auto_stimulus(0, 256)
        b.record_spikes(**kw)
        shards.append(b)
    gs = GpuShards(shards)
    for _ in range(passes):
        gs.pass_()
    torch.cuda.synchronize()
    with _gpu(*shape) as whole:
        whole.record_spikes(**kw)
        whole.encode_traversal(passes)
        want, counts = whole.spikes(), whole.spike_counts()
        assert want["info"]["spikes_seen"] > 5000 and want["info"]["passes_recorded"] == passes
        for r, b in enumerate(shards):
            got = b.spikes()
            assert got["info"] == want["info"], r
            assert np.array_equal(got["passes"], want["passes"]) and np.array_equal(got["raster"], want["raster"]), r
            assert np.array_equal(b.spike_counts(), counts), r
            assert np.array_equal(b.last_fired(), whole.last_fired()), r
    for b in shards:
        b.close()


# ---- 9. invalid arguments --------------------------------------------------------------------------------------
def test_invalid_arguments(gpu, shape1):
    import abnn_amd
    from abnn_amd import _lib, spikes

    lists, meta, _ = shape1
    lib = _lib.load()
    with _gpu(*SHAPE1) as g:
        h = g._h
        info, one = _lib.SpikesInfo(), np.zeros(4, dtype=np.uint64)
        # any call but start with no recorder
        for status in (lib.abnn_spikes_stop(h), lib.abnn_spikes_clear(h, 0), lib.abnn_spikes_get_info(h, C.byref(info)),
                       lib.abnn_spikes_read_passes(h, 0, 0, one.ctypes.data),
                       lib.abnn_spikes_read_raster(h, 0, 0, one.ctypes.data),
                       lib.abnn_spikes_read_counts(h, 0, 0, one.ctypes.data)):
            assert status == 1
        bad = {"reserved": _lib.SpikesConfig(10, 1, 0, 0, 0, (C.c_uint32 * 2)(0, 1)),
               "pass_capacity 0": spikes.config(10, 0),
               "range above N_NRN": spikes.config(10, 1, neurons=(N1 - 3, 4)),
               "range overflowing u32": spikes.config(10, 1, neurons=(0xFFFFFFFF, 2))}
        assert lib.abnn_spikes_start(h, None) == 1
        for what, cfg in bad.items():
            assert lib.abnn_spikes_start(h, C.byref(cfg)) == 1, what
            assert lib.abnn_spikes_get_info(h, C.byref(info)) == 1, what  # a failed start leaves no recorder
        # ... and the handle usable
        g.encode_traversal(4)
        g.record_spikes(raster=1 << 16, passes=16, neurons=(N1 - 4, 4))  # a range ending at N_NRN is fine
        g.record_spikes(raster=1 << 16, passes=16)  # counts off
        g.encode_traversal(4)
        _same(g.spikes(), spikes.reference(lists[4:8], meta[4:8], spikes.config(1 << 16, 16)))
        assert lib.abnn_spikes_get_info(h, None) == 1
        assert lib.abnn_spikes_read_passes(h, 0, 1, None) == 1
        assert lib.abnn_spikes_read_raster(h, 0, 1, None) == 1
        with pytest.raises(abnn_amd.AbnnError) as err:  # counts off
            g.spike_counts()
        assert err.value.status == 1
        g.record_spikes(raster=0, passes=1, neurons=(300, 7), counts=True)
        assert g.spike_counts().shape == (7,) and g.spike_counts(302, 2).shape == (2,)
        for first, n in ((299, 1), (300, 8), (307, 1), (0, 1)):  # absolute ids outside the selected range
            with pytest.raises(abnn_amd.AbnnError) as err:
                g.spike_counts(first, n)
            assert err.value.status == 1, (first, n)


# ---- the C++ mirrors and the engine path ------------------------------------------------------------------------
def test_cpp_spikes(gpu):
    from abnn_amd.build import build_spikes_test

    prog = build_spikes_test()
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    lines = r.stdout.strip().splitlines()
    assert lines, (r.returncode, r.stderr[-2000:])
    res = json.loads(lines[-1])
    assert r.returncode == 0 and res["ok"], (res, r.stderr[-2000:])
    assert res["passes"] == 16 and res["oracle_spikes"] == sum(SHAPE1_LENGTHS)
    assert res["engine_passes"] == 300 and res["engine_spikes"] > 0
