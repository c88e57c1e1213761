"""Sequences of record writers and passes on one handle, against the CPU oracle.

Every writer of the records (upload, build_graph, the edit's KILL and weight
ops, the reorder, a snapshot restore, the structural update) redoes or drops
its share of the handle's bookkeeping (DESIGN.md §9 "Who redoes what").  The
per-feature tests apply one writer and compare with a second GPU handle that
was uploaded to, which redoes everything.  Here writers follow each other with
no upload in between, and after every operation the handle equals the oracle
with the numpy host rules on bits: records, lastFired, scalars, rBar, the
statistics' differences, lastVisited, visited events, structural updates, the
census's tombstones, the device-side readers, and for sweep_indexed the src
index's state against the test's own book (scenario_helpers.Scenario).

a. every ordered pair of ten writers, per kind; b. seeded walks over the whole
vocabulary; c. the named sequences.  tests/test_scenario_model.py checks on the
CPU that all of them stay busy.  A failure prints the kind, the seed and the
operations so far; scenario_helpers.replay(kind, seed, upto) runs a prefix.
Sharded handles are not covered here.
"""
import pytest

import scenario_helpers as S

pytestmark = pytest.mark.gpu


@pytest.fixture
def env(monkeypatch):
    """The handle reads ABNN_INDEXED / ABNN_INDEX_AFTER when it is made (as tests/test_gpu_indexed.py)."""
    def for_kind(kind):
        if kind == "sweep_indexed":
            for k, v in S.INDEXED_ENV.items():
                monkeypatch.setenv(k, v)
    return for_kind


# ---- a. ordered pairs ---------------------------------------------------------------------------
@pytest.mark.parametrize("a", S.WRITERS)
@pytest.mark.parametrize("kind", S.KINDS)
def test_ordered_pairs(gpu, env, kind, a):
    """Three passes, capture, two passes, A, B, then passes until a structural
    update has run and two more (sweep_indexed: four passes, indexed by the
    book): every B after this A, a fresh pair each."""
    env(kind)
    for b in S.WRITERS:
        if (kind, a, b) in S.EXCLUDED:
            continue
        scn = S.run_pair(kind, a, b)
        assert len(scn.log) == len(S.pair_ops(kind, a, b))
        if kind == "sweep_indexed":
            assert sum(e["indexed"][-1] for e in scn.log[S.PAIR_HEAD:]) >= 3, (a, b)


# ---- b. seeded walks ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind,seed", [(k, s) for k in S.KINDS for s in S.WALK_SEEDS[k]])
def test_walk(gpu, env, kind, seed):
    env(kind)
    scn = S.run_walk(kind, seed)
    assert len(scn.log) + scn.skipped == S.WALK_OPS and scn.skipped * 10 <= S.WALK_OPS


# ---- c. named sequences -------------------------------------------------------------------------
def _named(env, name, kind):
    env(kind)
    scn = S.run_named(name, kind)
    assert len(scn.log) == len(S.NAMED[name][1])
    return scn


@pytest.mark.parametrize("kind", S.NAMED["kill_reorder_kill_update"][0])
def test_kill_reorder_kill_then_structural_update(gpu, env, kind):
    """The KILL's tally, zeroed and recounted by the reorder, added to by the
    second KILL, read by the structural update's O(D) fill."""
    _named(env, "kill_reorder_kill_update", kind)


@pytest.mark.parametrize("kind", S.NAMED["records_restore_onto_grown_half_full"][0])
def test_records_restore_onto_another_n_syn_with_grown_records_waiting(gpu, env, kind):
    """The records of pass 2 come back at pass 5: n_syn has changed, the odd
    pass's grown records wait, and the next update appends them to the
    restored records."""
    _named(env, "records_restore_onto_grown_half_full", kind)


@pytest.mark.parametrize("kind", S.NAMED["upload_over_killed_chunks"][0])
def test_partial_uploads_over_chunks_a_kill_tallied(gpu, env, kind):
    """Slices with planted tombstones across a chunk boundary, inside the last
    chunk and across m = n_syn - D, over chunks whose tally a KILL had raised."""
    _named(env, "upload_over_killed_chunks", kind)


def test_reorders_across_the_sweep_end_under_an_index(gpu, env):
    """Shuffle, sort and inverse permutation carry records across E = 100 096
    of 120 000 while an index over [0, E) exists: dropped each time, built
    again one pass later, the passes after it indexed."""
    scn = _named(env, "reorder_across_the_sweep_end", "sweep_indexed")
    assert all(e["indexed"][-1] for e in scn.log if e["name"] == "passes")


def test_state_restore_then_an_indexed_pass(gpu, env):
    """A restore of the state alone writes no record: the index stays and the
    very next pass is indexed, its bitmap rebuilt from the restored lastFired.
    Six passes lie between the capture and the restore, so the pass before the
    restore has built the next bitmap from the spike lists: a restore that
    kept that bitmap would gate other events (pre_gated differs)."""
    scn = _named(env, "state_restore_then_indexed_pass", "sweep_indexed")
    assert scn.log[4]["indexed"] == [True]
