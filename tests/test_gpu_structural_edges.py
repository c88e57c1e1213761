"""GPU parity of the structural update (capi.hip structural_update, kernels.hip
launch_structural_update) at its block, tail and capacity edges: the removal
alone on the catalogue of tests/structural_helpers.py against the numpy
restatement of abnn.h and against the oracle; growth against a saturating
capacity and at the grown-slot array's block edges; the passes after an update
in both modes (random mode reads the src mirror the update moved).  Everything
is integer or bit-exact fp32: every comparison is array_equal on the uint32
view, or ==.  tests/test_structural_model.py checks the expected values and
the patterns' properties without a GPU."""
import numpy as np
import pytest

import structural_helpers as H
from test_gpu_plasticity import _pair, _same

pytestmark = pytest.mark.gpu


def _bits_equal(a, b):
    return len(a) == len(b) and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 3. the removal alone -------------------------------------------------------------------

def _removal_alone(name, n, oracle=True):
    """No events, an update after every pass, nothing pruned by a pass and
    nothing grown: the pass visits nothing and its commit removes the uploaded
    tombstones (the upload recounts the tally)."""
    import abnn_amd
    from oracle import oracle as O

    syn, _, d = H.case(name, n)  # asserts the pattern's property
    want = H.removal_reference(syn)
    kw = dict(syn_capacity=n, compact_every=1, w_prune=1e-30, p_new=0.0)
    g = abnn_amd.Brain(256, 256, H.N_HIDDEN, n, 0, **kw)
    g.upload_synapses(syn)
    o = None
    if oracle:
        o = O.OracleBrain(256, 256, H.N_HIDDEN, n, 0, **kw)
        o.set_synapses(syn)
    for k in (1, 2):  # the second update: no tombstone is left and the tally was cleared, nothing changes
        g.encode_traversal(1)
        assert g.structural_updates() == k
        assert g.n_syn() == len(want) == d["m"], (name, n, k)
        assert _bits_equal(g.download_synapses(), want), (name, n, k)
        if o is not None:
            o.pass_serial()
            _same(g, o, f"{name} {n} update {k}")
    assert g.scalars()["clock"] == 0  # nothing visited: no tick


@pytest.mark.parametrize("name,n", H.cases(big=False))
def test_removal_alone(gpu, name, n):
    _removal_alone(name, n)


def test_removal_alone_more_than_1024_blocks(gpu):
    """8 396 801 records, every other one dead: 1026 hole blocks and 1026 tail
    blocks, so the second slice of k_swap_scan1/2 (the `lower` sum) and the
    second round of k_swap_tail's loop run.  Uploads 134 MB; the one case that
    may take more than a couple of seconds: measured 1.2 s on an MI355X, the
    oracle comparison included (so it stays)."""
    _removal_alone("every_other_big", H.BIG)


# ---- 4. growth against capacity -------------------------------------------------------------

def _dst_w_at(g, index):
    """The {dst, w} words of device record `index` read through the device
    layout (test-only raw read; the handle then rebuilds its bitmap every
    pass, so call it last)."""
    import ctypes as C

    with open("/proc/self/maps") as f:  # the HIP runtime the library loaded, not a second one
        loaded = {line.split()[-1] for line in f if "libamdhip64.so" in line}
    assert len(loaded) == 1, loaded
    hip = C.CDLL(loaded.pop())
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    base, nbytes, eb = g.synapse_layout()["arrays"]["dst_w"]
    assert eb == 8 and (index + 1) * 8 <= nbytes
    out = (C.c_uint32 * 2)()
    assert hip.hipMemcpy(out, base + index * 8, 8, 2) == 0  # hipMemcpyDeviceToHost
    return tuple(out)


def _grow_pair(**kw):
    return _pair(**dict(dict(p_new=1.0), **kw))


def _run_checked(g, o, passes, ce, expect_cut):
    """`passes` passes, compared every pass.  Returns whether at one update at
    least the period's grown attempts (p_new = 1: the spikes) exceeded the room
    capacity - (n_syn - D), on the oracle's side, and n_syn == capacity after it."""
    cap = int(o.s.dims.syn_capacity)
    cut, fired0 = False, 0
    for k in range(passes):
        before = o.syn.copy()
        tombs_before = int(H.is_tomb(before).sum())
        pruned0 = o.stats()["pruned"]
        g.encode_traversal(1)
        o.pass_serial()
        _same(g, o, f"pass {k}")
        assert g.n_syn() <= cap
        if (k + 1) % ce == 0:
            st = o.stats()
            attempts, fired0 = st["fired"] - fired0, st["fired"]
            D = tombs_before + st["pruned"] - pruned0
            room = cap - (len(before) - D)
            if attempts > room:
                cut = True
                assert g.n_syn() == cap == int(o.s.dims.n_syn), f"pass {k}: {attempts} attempts, room {room}"
    assert g.stats() == o.stats()
    assert cut == expect_cut
    # the first record past the capacity (the arrays' zero padding) was never written:
    # a dropped slot's record is not stored anywhere, not even where no download looks
    assert _dst_w_at(g, cap) == (0, 0)
    return cut


# The oracle's numbers (120 000 records, 256 stimulated inputs): the first
# spikes are pass 3's, 2560 of them (the whole budget), nothing pruned yet; so
# the update after pass 3 meets 2560 attempts and a room of cap_extra.  With
# compact_every = 2 pass 3 is its period's second pass: its slots are 2560 ..
# 5119, i.e. 512 in slot block 2 and all of blocks 3 and 4.  cap_extra 0, 1, 7
# cut inside block 2, the first block holding used slots (`below` = 0 in
# k_append_grown); 1000 cuts inside block 3, the second one (below = 512, 488
# of its records stay).  With compact_every = 1 the slots are 0 .. 2559 and
# cap_extra = 1500 cuts inside the period's second 1024-slot block proper
# (below = 1024, 476 stay).  Later updates have room: pruning freed 38 000.
@pytest.mark.parametrize("cap_extra,w_prune,ce", [(0, 0.105, 2), (1, 0.105, 2), (7, 0.105, 2), (1000, 0.105, 2),
                                                   (1500, 0.105, 1), (1, 0.0, 2)])
def test_growth_capacity_cut(gpu, cap_extra, w_prune, ce):
    g, o = _grow_pair(cap_extra=cap_extra, w_prune=w_prune, compact_every=ce)
    _run_checked(g, o, 8, ce, expect_cut=True)


def test_growth_capacity_cut_random_mode(gpu):
    """cap_extra = 7 in random mode (60 000 picks).  With w_prune = 0.105 the
    oracle's random-mode pass 3 prunes 3773 records beside its 2560 spikes, so
    the room (3780) exceeds the attempts and nothing is cut; the cut needs
    w_prune = 0 there (room 7 against 2560 attempts)."""
    g, o = _grow_pair(mode=1, events=60_000, cap_extra=7, w_prune=0.0)
    _run_checked(g, o, 8, 2, expect_cut=True)


# 1, 6, exactly 1024, 2049 and 2560 grown slots; max_spikes also caps the pass's spikes
@pytest.mark.parametrize("ce,max_spikes", [(1, 1), (2, 3), (2, 512), (3, 683), (1, 2560)])
def test_growth_slot_array_sizes(gpu, ce, max_spikes):
    assert ce * max_spikes == {(1, 1): 1, (2, 3): 6, (2, 512): H.SLICE, (3, 683): 2 * H.SLICE + 1,
                               (1, 2560): 2560}[(ce, max_spikes)]
    g, o = _grow_pair(cap_extra=20_000, compact_every=ce, max_spikes=max_spikes)
    for k in range(8):
        g.encode_traversal(1)
        o.pass_serial()
        _same(g, o, f"pass {k}")
    st = g.stats()
    assert st == o.stats() and st["grown"] > 0


def test_every_record_dies_while_grown_records_wait(gpu):
    """compact_every = 2, nothing pruned by the passes.  The first spikes are
    pass 3's, so the period of passes 4 and 5 is the first whose first pass
    grows records: after pass 4 every record is lesioned (the edit keeps the
    tally and leaves the grown slots alone), pass 5 visits tombstones only, and
    its update has m = 0: the array is the grown records of the two passes,
    from index 0."""
    from abnn_amd import edit as E

    g, o = _grow_pair(w_prune=0.0, compact_every=2)
    for k in range(5):
        g.encode_traversal(1)
        o.pass_serial()
        _same(g, o, f"pass {k}")
    grown0, n0 = o.stats()["grown"], g.n_syn()
    head = g.edit("kill")
    assert head["killed"] == n0
    dead, _ = E.reference(o.syn, E.config("kill"), o.n_neuron())
    o.set_synapses(dead)
    _same(g, o, "lesioned")
    g.encode_traversal(1)
    o.pass_serial()
    _same(g, o, "the update with m = 0")
    grown = o.stats()["grown"] - grown0
    assert g.n_syn() == grown > 0
    syn = g.download_synapses()
    assert not H.is_tomb(syn).any() and (syn["w"] == np.float32(0.5)).all()  # w_init: grown records only
    for k in range(3):
        g.encode_traversal(1)
        o.pass_serial()
        _same(g, o, f"after, pass {k}")
    assert g.stats() == o.stats()


# ---- 5. the passes after an update, both modes ----------------------------------------------

@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", [H.MID, 120_000])
@pytest.mark.parametrize("name", H.PASS_PATTERNS)
def test_passes_after_update(gpu, name, n, mode):
    """The update by pass 1 on an uploaded pattern (direct path, scan path,
    almost all), then four passes on the moved records.  Random mode picks
    through the src mirror move_record moved; downloads do not read it."""
    events = n if mode == 0 else n // 2
    g, o = _pair(mode, n_syn=n, events=events, cap_extra=0, w_prune=1e-30, p_new=0.0, compact_every=1)
    syn, dead, d = H.case(name, n)
    g.upload_synapses(syn)
    o.set_synapses(syn)
    for k in range(5):
        g.encode_traversal(1)
        o.pass_serial()
        _same(g, o, f"{name} pass {k}")
        assert g.n_syn() == d["m"]
        assert g.visited_events() == (min(g.n_syn(), (events + 255) // 256 * 256) if mode == 0 else events)
    st = g.stats()
    assert st == o.stats()
    assert st["events"] == (min(n, (events + 255) // 256 * 256) if mode == 0 else events) + 4 * g.visited_events()
    assert g.structural_updates() == 5
