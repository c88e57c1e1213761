"""The crafted high-id graph (tests/high_id_helpers.py) on the CPU oracle alone:
the conditions that make tests/test_gpu_high_ids.py meaningful.  A graph that
left an id class without recent neurons, or the filter without false
positives to reject, would let those tests pass while proving nothing."""
import numpy as np
import pytest

import high_id_helpers as H

N_NRN = 2**24 - 2
PASSES = 12


def _oracle(n_nrn, **over):
    from oracle import oracle as O

    syn = H.high_id_graph(n_nrn)
    o = O.OracleBrain(256, 256, n_nrn - 512, len(syn), len(syn), **over)
    o.set_synapses(syn)
    o.set_auto_stimulus(0, 256)
    return o


@pytest.mark.parametrize("over", [{}, dict(max_spikes=200_000)], ids=["default", "budget-huge"])
def test_crafted_graph_reaches_every_id_class(over):
    parts = H.high_id_parts(N_NRN)
    decoys, f2_decoys = parts["decoys"], parts["f2_decoys"]
    assert len(decoys) >= 40 and len(f2_decoys) >= 8
    n_classes = (N_NRN - 1 >> H.CLASS_LOG2) + 1
    assert n_classes == 64
    o = _oracle(N_NRN, **over)
    src = o.syn["src"].astype(np.int64)  # (the sweep changes no src)
    src_class = src >> H.CLASS_LOG2
    all_decoys_alias, f2_alias = False, 0
    for k in range(PASSES):
        now = o.clock
        lf0 = o.last_fired.copy()
        lf0[:256] = now  # the stimulus is stamped at pass start
        recent = H.recent_mask(lf0, now)
        g1 = o.stats()["pre_gated"]
        o.pass_threaded(nthreads=16)
        g1 = o.stats()["pre_gated"] - g1
        if k < 5:  # the creation zeros: every neuron is recent (the model of all 2^24 ids: pass 5 only)
            assert recent.all() and g1 == len(src), k
            continue
        ids = np.flatnonzero(recent)
        model = H.filter_model(ids)
        hit = H.passes_filter(model, src)
        gated = recent[src]
        assert not (gated & ~hit).any(), f"pass {k}: the filter model drops a recent src"
        assert int((hit & gated).sum()) == g1, f"pass {k}: pre-gated count"
        if k < 6:  # the creation zeros are still recent: every neuron is
            continue
        assert not recent[decoys].any(), f"pass {k}: a decoy was stamped"
        assert np.unique(ids >> H.CLASS_LOG2).size == n_classes, f"pass {k}: a class without recent neurons"
        assert np.unique(src_class[gated]).size == n_classes, f"pass {k}: a class without pre-gated records"
        assert int((hit & ~gated).sum()) > 0, f"pass {k}: no false positive to reject"
        d_hit = H.passes_filter(model, decoys)
        all_decoys_alias |= bool(d_hit.all())
        # the decoys that the Bloom filter passes too: only the exact bitmap rejects them
        both = H.passes_filter(model, f2_decoys) & H.passes_f2(H.f2_model(ids), f2_decoys)
        f2_alias = max(f2_alias, int(both.sum()))
    assert all_decoys_alias, "no pass in which every alias decoy passes the blocked filter"
    assert f2_alias >= 8, "no pass in which several Bloom-covered decoys pass both filters"
    assert o.stats()["fired"] > 0 and o.stats()["updated"] > o.stats()["fired"]


@pytest.mark.parametrize("n_nrn", [2**18 + 70, 2**23 + 70, 2**25 + 77])
def test_crafted_graph_at_the_other_sizes(n_nrn):
    """The first sizes with t != 0 and with x = 1, and the raw launcher's ids
    above 24 bits: from pass 6 on every class holds recent neurons and
    pre-gated records, and the model agrees with the oracle's count."""
    n_classes = (n_nrn - 1 >> H.CLASS_LOG2) + 1
    o = _oracle(n_nrn)
    src = o.syn["src"].astype(np.int64)
    for k in range(8):
        now = o.clock
        lf0 = o.last_fired.copy()
        lf0[:256] = now
        recent = H.recent_mask(lf0, now)
        g1 = o.stats()["pre_gated"]
        o.pass_threaded(nthreads=16)
        if k < 5:  # the creation zeros: every neuron is recent
            assert recent.all() and o.stats()["pre_gated"] - g1 == len(src), k
            continue
        ids = np.flatnonzero(recent)
        hit = H.passes_filter(H.filter_model(ids), src)
        assert not (recent[src] & ~hit).any(), k
        assert int((hit & recent[src]).sum()) == o.stats()["pre_gated"] - g1, k
        if k >= 6:
            assert np.unique(ids >> H.CLASS_LOG2).size == n_classes, k
            assert np.unique(src[recent[src]] >> H.CLASS_LOG2).size == n_classes, k


def test_filter_model_notices_a_dropped_rotation_and_a_dropped_x_bit():
    """The model is sharp enough for the two code mutations that matter above
    2^18: without the high image's rotation recent ids stop passing, and a
    decode that forgets the x bit maps ids >= 2^23 elsewhere."""
    ids = H.fixed_ids(N_NRN)
    low, high = H.filter_model(ids)
    assert H.passes_filter((low, high), ids).all()
    jh = H.filter_slot(ids)[3]
    assert not H.passes_filter((low, low), ids[(jh % 32) != 0]).all()  # (unrotated, the high image is the low one)
    lo, hi = H._src_code(ids)
    assert np.array_equal(H._code_src(lo, hi), ids.astype(np.uint64))
    assert not np.array_equal(H._code_src(lo, hi & ~np.uint64(32)), ids.astype(np.uint64))
