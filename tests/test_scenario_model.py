"""The scenarios of tests/test_gpu_scenarios.py on the oracle side alone
(scenario_helpers with g = None): they are inputs, and only worth running on
the GPU while they stay busy.  Every pair sequence, walk and named sequence
runs here, and the conditions below hold for the seeds, ranges and bands in
scenario_helpers; when one stops holding, pick others there, do not loosen it.

sweep_indexed has no structural update and a constant n_syn (no plasticity,
compact_every = 0: a KILL's tombstones stay), so three conditions take the form
that exists there: "a structural update after a reorder" is an indexed pass
after a reorder, the pair sequences' n_syn does not change, and no restore
meets another n_syn.
"""
import collections
import functools

import pytest

import scenario_helpers as S

PLASTIC = ("sweep_plastic", "random_plastic")


def busy(scn):
    """Writers change something: every kill kills, every weight edit changes a
    weight, every reorder but the compaction (which only moves tombstones)
    leaves a record at another index, every restore of records differs from
    what it replaces."""
    for e in scn.log:
        n, what = e["name"], f"{scn.kind} {scn.seed}: {e['op']}"
        if n.startswith("kill"):
            assert e["killed"] > 0, what
        if n in ("affine", "draw"):
            assert e["changed"] > 0, what
        if n == "perm" or (n.startswith("reorder") and n != "reorder_none"):
            assert e["moved"] > 0, what
        if n in ("restore_records", "restore_both"):
            assert e["differs"], what


def flags(scn):
    f = set()
    for e in scn.log:
        if e.get("after_reorder"):
            f.add("update after a reorder")
        if e["name"] in ("restore_records", "restore_both") and e["n_before"] != e["n_after"]:
            f.add("restore onto another n_syn")
        if e.get("over_killed"):
            f.add("kill, then an upload over the same chunk")
        if e["name"] == "reorder_none" and e["tombstones"] > 0:
            f.add("compaction with tombstones")
    return f


def test_the_pair_list():
    combos = [(k, a, b) for k in S.KINDS for a in S.WRITERS for b in S.WRITERS]
    assert len(S.WRITERS) == 10 and len(combos) == 300
    assert set(S.EXCLUDED) <= set(combos) and len(S.EXCLUDED) <= 10
    assert len(combos) - len(S.EXCLUDED) >= 290


@pytest.mark.parametrize("a", S.WRITERS)
@pytest.mark.parametrize("kind", S.KINDS)
def test_pair_sequences_stay_busy(kind, a):
    seen = set()
    for b in S.WRITERS:
        if (kind, a, b) in S.EXCLUDED:
            continue
        scn = S.run_pair(kind, a, b, gpu=False)
        assert scn.skipped == 0 and len(scn.log) == len(S.pair_ops(kind, a, b))
        busy(scn)
        seen |= flags(scn)
        tail = scn.log[S.PAIR_HEAD:]
        what = f"{kind}: {a}, {b}"
        assert sum(e["stats"]["fired"] for e in tail) > 0 and sum(e["stats"]["updated"] for e in tail) > 0, what
        if kind in PLASTIC:
            assert sum(e["su"] for e in tail) >= 1, what
            assert sum(e["stats"]["pruned"] for e in scn.log) > 0 and sum(e["stats"]["grown"] for e in scn.log) > 0, what
            assert len({e["n_syn"] for e in scn.log}) > 1, what
        else:
            assert sum(e["indexed"][-1] for e in tail) >= 3, what  # the tail is indexed (its first pass after a writer that drops the index streams)
    if a in ("kill_dst", "kill_w", "upload_slice"):
        assert "compaction with tombstones" in seen, (kind, a)


@functools.lru_cache(maxsize=None)
def _walk(kind, seed):
    return S.run_walk(kind, seed, gpu=False)


@pytest.mark.parametrize("kind", S.KINDS)
def test_walks_stay_busy(kind):
    seeds = S.WALK_SEEDS[kind]
    assert len(seeds) >= 6 and len(set(seeds)) == len(seeds)
    ran, seen = collections.Counter(), set()
    for seed in seeds:
        scn = _walk(kind, seed)
        assert len(scn.log) + scn.skipped == S.WALK_OPS
        assert scn.skipped * 10 <= S.WALK_OPS, f"{kind} {seed}: {scn.skipped} draws skipped"
        busy(scn)
        ran.update(e["name"] for e in scn.log)
        seen |= flags(scn)
    assert 0.25 <= ran["passes"] / (len(seeds) * S.WALK_OPS) <= 0.42, ran["passes"]  # about a third of the draws
    for name in S.VOCABULARY:
        if name == "flavour" and kind == "random_plastic":  # the sweep kinds only
            assert ran[name] == 0
            continue
        assert ran[name] >= 2, f"{kind}: {name} ran {ran[name]} times over the seeds"
    want = {"update after a reorder", "kill, then an upload over the same chunk", "compaction with tombstones"}
    if kind in PLASTIC:
        want.add("restore onto another n_syn")
    assert want <= seen, f"{kind}: {want - seen}"


@pytest.mark.parametrize("kind", S.KINDS)
def test_walks_are_deterministic(kind):
    seed = S.WALK_SEEDS[kind][0]
    again = S.run_walk(kind, seed, gpu=False)
    assert again.ops == _walk(kind, seed).ops and again.skipped == _walk(kind, seed).skipped
    prefix = S.replay(kind, seed, 7, gpu=False)
    assert prefix.ops == again.ops[:7]


@pytest.mark.parametrize("name", S.NAMED)
def test_named_sequences_stay_busy(name):
    kinds, ops = S.NAMED[name]
    for kind in kinds:
        scn = S.run_named(name, kind, gpu=False)
        assert scn.skipped == 0 and len(scn.log) == len(ops)
        busy(scn)
        log = {e["name"]: e for e in scn.log}
        if name == "kill_reorder_kill_update":
            assert log["su_pass"]["su"] == 1 and scn.log[3]["tombstones"] > scn.log[1]["tombstones"] > 0
        if name == "records_restore_onto_grown_half_full":
            r = log["restore_records"]
            assert r["n_before"] != r["n_after"] and int(scn.o.s.pass_index) % 2 == 0
            assert scn.log[2]["stats"]["fired"] > 0  # (spikes of the odd pass before the restore: its grown records wait)
            assert log["su_pass"]["stats"]["grown"] > 0 and log["su_pass"]["op"] == ("passes", 1)
        if name == "upload_over_killed_chunks":
            ups = [e for e in scn.log if e["name"] == "upload_slice"]
            assert len(ups) == 3 and all(e["over_killed"] and e["planted"] > 0 for e in ups)
            first, n = ups[0]["first"], ups[0]["n"]
            assert first // S.CHUNK != (first + n - 1) // S.CHUNK  # across a chunk boundary
            first, n = ups[1]["first"], ups[1]["n"]
            assert first // S.CHUNK == (first + n - 1) // S.CHUNK == (ups[1]["n_syn"] - 1) // S.CHUNK  # in the last chunk
            m = scn.log[3]["n_syn"] - scn.log[3]["tombstones"]  # before the third upload
            assert ups[2]["first"] < m < ups[2]["first"] + ups[2]["n"]
        if name == "reorder_across_the_sweep_end":
            assert all(e["indexed"][-1] for e in scn.log if e["name"] == "passes")
            assert scn.shape[1] - scn.shape[2] >= 19_000  # live records past the sweep's end
        if name == "state_restore_then_indexed_pass":
            assert scn.log[4]["indexed"] == [True]  # the restore of the state alone keeps the index
