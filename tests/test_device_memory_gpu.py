"""Who owns the library's device memory (csrc/pool.h, DESIGN.md §9 "Device
memory"), checked through abnn_debug_live_allocations: the device allocations
the library made and has not freed yet.  Every handle's destroy gives back
all it took, repeated calls reuse their scratch, a replaced buffer is freed
at once, and a refused call takes nothing.  The shape is tiny on purpose:
nothing here depends on size (256 / 256 / 488 neurons, 20,001 records: the
last one in no 16-byte pair)."""
import ctypes as C
import gc
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NI, NO, NH, N_SYN = 256, 256, 488, 20_001
N_NRN = NI + NO + NH
# every conditional buffer of abnn_brain_create: pruning and synaptogenesis on, visits tracked
KW = dict(seed=13, track_visits=1, w_prune=0.105, p_new=0.35, w_init=0.5, compact_every=4,
          syn_capacity=N_SYN + 4_000)
RASTER, PASSES = 1 << 14, 64


def live() -> int:
    from abnn_amd import _lib

    return int(_lib.load().abnn_debug_live_allocations())


@pytest.fixture(autouse=True)
def _settled():
    gc.collect()  # a handle an earlier test dropped goes now, not in the middle of a count


def pointer_members(header: str, struct: str) -> int:
    """The device buffers of a scratch struct of csrc/: its pointer members,
    an array of pointers counting once per entry."""
    with open(os.path.join(ROOT, "abnn_amd", "csrc", header)) as f:
        body = re.search(r"struct %s \{(.*?)\n\};" % struct, f.read(), re.S).group(1)
    n = 0
    for m in re.finditer(r"^\s*[\w ]+\*\s*\w+(?:\[(\d+)\])?\s*(?:=|;)", body, re.M):
        n += int(m.group(1) or 1)
    return n


def _brain():
    import abnn_amd

    return abnn_amd.Brain(NI, NO, NH, N_SYN, N_SYN, **KW)


def _frames(n, seed=5):
    rng = np.random.default_rng(seed)
    return rng.random((n, NI), dtype=np.float32), rng.random((n, NO), dtype=np.float32)


def _module_calls(b, degree_neurons=(256, 64), hops_seeds=(0, 16)):
    """Once each: the census-style modules, the recorder and corr in its three
    modes, a PERM reorder, a snapshot's life and an engine's."""
    import abnn_amd

    b.census(64, 0.0, 1.0)
    b.degrees(neurons=degree_neurons, what=("out", "in_w"))
    b.select(dst=(256, 64), capacity=100)
    b.edit("scale_dst", dst=(256, 64), plane=np.full(64, 1.01, np.float32))  # a SCALE op: the plane is staged
    b.hops(hops_seeds, max_hops=8)
    b.record_spikes(RASTER, PASSES)
    b.encode_traversal(5)
    for mode in ("pop", "pairs", "synapses"):
        b.correlate(mode, a=(0, 64), b=(256, 64), max_lag=4)
    b.reorder(perm=np.arange(b.n_syn(), dtype=np.uint32)[::-1])  # PERM: both temporaries are staged
    with b.snapshot() as snap:
        b.encode_traversal(2)
        snap.diff(64, -0.05, 0.05)
        snap.restore()
    xin, xex = _frames(4)
    with abnn_amd.LearnEngine(b, win_size=5, trace_passes=8) as e:
        e.run(xin, xex)
        e.set_census(16, 0.0, 1.0, every=1, capacity=2)
        e.set_census(16, 0.0, 1.0, every=1, capacity=8)
        e.run(xin[:2], xex[:2])
        e.state()


def _whole_life():
    from abnn_amd import graph

    with _brain() as b:
        b.build_graph(graph.recipe(NI, NO, NH, N_SYN, seed=3))
        b.set_auto_stimulus(0, NI)
        b.encode_traversal(9)  # structural updates after passes 4 and 8
        assert b.structural_updates() == 2
        _module_calls(b)
        assert live() > 0


def test_destroy_returns_everything(gpu):
    """A brain that used every module, a snapshot and an engine; then again in
    the same process: the counter is back where it was both times."""
    before = live()
    _whole_life()
    assert live() == before
    _whole_life()
    assert live() == before


@pytest.fixture()
def used():
    """A brain after its first round of calls: every scratch exists."""
    with _brain() as b:
        b.build_random_graph(21)
        b.set_auto_stimulus(0, NI)
        b.encode_traversal(3)
        _module_calls(b)
        yield b


def test_steady_state_does_not_grow(gpu, used):
    """The same calls with the same arguments: the scratch is reused and the
    temporaries are freed, whether or not a structural update fell between."""
    at = live()
    _module_calls(used)
    assert live() == at
    _module_calls(used)
    assert live() == at


def test_replacement_not_accumulation(gpu, used):
    b = used
    at = live()
    # the recorder restarted larger, then corr: its rows and tallies are replaced
    b.stop_spikes()
    n_rec = pointer_members("spikes.h", "SpikeRecorder")
    assert n_rec == 4
    assert live() == at - (n_rec - 1)  # (a raster, no counts: three of the four)
    b.record_spikes(2 * RASTER, 2 * PASSES)
    b.encode_traversal(2)
    b.correlate("pop", max_lag=4)
    assert live() == at
    b.record_spikes(2 * RASTER, 2 * PASSES, counts=True)  # a restart frees the old recorder first
    assert live() == at + 1
    b.encode_traversal(3)
    b.correlate("pairs", a=(0, 64), b=(256, 64), max_lag=4)
    assert live() == at + 1
    b.stop_spikes()
    assert live() == at + 1 - n_rec
    b.record_spikes(RASTER, PASSES)
    assert live() == at
    # larger results than before: the result buffers grow in place
    b.degrees()
    b.hops((0, 16), max_hops=64)
    assert live() == at
    # the reorder scratch goes at once and comes back with the next reorder
    n_reorder = pointer_members("reorder.h", "ReorderScratch")
    assert n_reorder >= 6
    b.reorder_release()
    assert live() == at - n_reorder
    b.reorder_release()
    assert live() == at - n_reorder
    b.reorder("dst")
    assert live() == at


def test_refusals_leak_nothing(gpu, used):
    """An invalid config, a null argument and a wrong `words` to each module
    (their statuses are checked elsewhere): nothing is taken."""
    from abnn_amd import _lib, census, corr, degree, edit, hops, reorder, select, snapshot

    b, lib = used, _lib.load()
    h = b._h
    out = np.zeros(1 << 16, np.uint64)
    po = out.ctypes.data
    perm = np.arange(b.n_syn(), dtype=np.uint32)
    plane = np.ones(64, np.float32)
    cc, dc, sc = census.config(64, 0.0, 1.0), degree.config((256, 64)), select.config(dst=(256, 64))
    ec, rc = edit.config("scale_dst", dst=(256, 64)), reorder.config("perm")
    hc, kc = hops.config((0, 16), 8), corr.config("pop", max_lag=4)
    fc = snapshot.config(64, -0.05, 0.05)
    with b.snapshot() as snap:
        at = live()
        good = {
            "census": lambda c=cc, o=po, d=0: lib.abnn_census(h, c, o, lib.abnn_census_words(C.byref(cc)) + d),
            "degree": lambda c=dc, o=po, d=0: lib.abnn_degree(h, c, o, lib.abnn_degree_words(C.byref(dc), N_NRN) + d),
            "select": lambda c=sc, o=po, d=0: lib.abnn_select(h, c, 100, o, lib.abnn_select_words(C.byref(sc), 100) + d),
            "edit": lambda c=ec, o=po, d=0: lib.abnn_edit(h, c, plane.ctypes.data, 64 + d, o),
            "reorder": lambda c=rc, o=po, d=0: lib.abnn_reorder(h, c, perm.ctypes.data, o,
                                                                 lib.abnn_reorder_words(C.byref(rc), b.n_syn()) + d),
            "hops": lambda c=hc, o=po, d=0: lib.abnn_hops(h, c, o, lib.abnn_hops_words(C.byref(hc), N_NRN) + d),
            "corr": lambda c=kc, o=po, d=0: lib.abnn_corr(h, c, o, lib.abnn_corr_words(C.byref(kc)) + d),
            "diff": lambda c=fc, o=po, d=0: lib.abnn_snapshot_diff(h, snap._h, None, c, o,
                                                                    lib.abnn_snapshot_diff_words(C.byref(fc)) + d),
        }
        bad = {"census": census.config(0, 0.0, 1.0), "degree": degree.config((N_NRN, 8)),
               "select": select.config(dst=(N_NRN, 8)), "edit": edit.config("scale_dst", dst=(N_NRN, 8)),
               "reorder": reorder.config("perm", seed=7), "hops": hops.config((N_NRN, 8), 8),
               "corr": corr.config("pop", max_lag=4000), "diff": snapshot.config(0, -0.05, 0.05)}
        for name, fn in good.items():
            for what, status in (("config", fn(c=bad[name])), ("null", fn(o=None)), ("words", fn(d=1))):
                assert status != 0, (name, what)
                assert live() == at, (name, what)
            assert fn() == 0, name  # ... and the call they garbled is a good one
            assert live() == at, name
        assert lib.abnn_spikes_start(h, None) != 0
        assert lib.abnn_snapshot_create(h, None) != 0 and lib.abnn_engine_create(h, None, None) != 0
        assert live() == at
        # a start frees the old recorder first (abnn.h), so the refused config goes to a stopped one
        b.stop_spikes()
        at = live()
        assert lib.abnn_spikes_start(h, _lib.SpikesConfig(RASTER, 0, 0, 0, 0)) != 0  # pass_capacity 0
        assert lib.abnn_corr(h, kc, po, lib.abnn_corr_words(C.byref(kc))) != 0  # no recorder
        assert live() == at


def test_communicator_returns_everything(gpu):
    """A one-rank in-process group (no RCCL): one sharded pass, the visits'
    merge and its all-reduce, then the destroys."""
    from abnn_amd.shard import LocalGroup, ShardedBrain

    before = live()
    g = LocalGroup(1)
    sb = ShardedBrain(g.comm(0, 0), NI, NO, NH, N_SYN, N_SYN, device=0, track_visits=1)
    try:
        sb.brain.build_random_graph(4)
        sb.brain.set_auto_stimulus(0, NI)
        sb.step(2)
        sb.sync_visits()
        sb.brain.synchronize()
        assert live() > before
    finally:
        sb.brain.close()
        g.close()
    del sb, g
    assert live() == before
