"""Device-side snapshots on the GPU (abnn.h abnn_snapshot_*, csrc/snapshot.hip,
csrc/capi.hip).

Every comparison is bit-exact.  The diff against snapshot.reference over the two
downloads, word for word: the record-count edges of the CPU file, unequal sides
(through a structural update and a restore), a brain of many workgroup
iterations whose last record is in no 16-byte pair, every changed d equal at 1
and 4096 bins; the diff of two snapshots and the enqueue-only path; restore
against the state at the capture; restore-then-run against the run straight
after the capture in both modes, with track_visits, across a renormalisation,
inject_inputs and an abnn_engine_run call; the same with pruning and
synaptogenesis on; the parts; refusals; shards; the C++ mirror."""
import ctypes as C
import json
import socket
import subprocess

import numpy as np
import pytest

from snapshot_helpers import CONFIGS, N_NRN, NONE, SIZES, SPECIAL_PAIRS, UNEQUAL, invariants, pair, records

pytestmark = pytest.mark.gpu

F32 = np.float32
BIG = 3_000_001  # many workgroup iterations; the last record is in no 16-byte pair
SENTINEL = 0x5A5A5A5A5A5A5A5A
P = 9  # the contract's passes after the capture / the restore
HZ = 1e-12  # inject_inputs: p = hz * tick_ns * 1e9 * value = the value itself


def _brain(n_syn, events=100_000, **kw):
    import abnn_amd

    return abnn_amd.Brain(256, 256, 488, n_syn, events, **kw)


def _learner(n_syn=120_000, **kw):
    """A 256 / 256 / 488 brain whose passes spike and learn."""
    b = _brain(n_syn, n_syn, seed=13, **kw)
    b.build_random_graph(21)
    b.set_auto_stimulus(0, 256)
    return b


def _same_records(got, want, what=""):
    g, w = got.view(np.uint32).reshape(-1, 4), want.view(np.uint32).reshape(-1, 4)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero((g != w).any(axis=1))
    assert bad.size == 0, (what, bad.size, bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist())


def _diff_equals_reference(snap, then, now, what="", now_snap=None):
    """Every config of the small set: Snapshot.diff == snapshot.reference, word for word."""
    from abnn_amd import snapshot

    out = {}
    for name, args in CONFIGS.items():
        got = snap.diff(*args[:3], src=args[3], dst=args[4], now=now_snap)
        want = snapshot.reference(then, now, snapshot.config(*args))
        invariants(got)
        assert snapshot.to_words(got).tolist() == snapshot.to_words(want).tolist(), (what, name)
        out[name] = got
    return out


def _state(b):
    return {"syn": b.download_synapses(), "lf": b.last_fired(), "lv": b.last_visited(), "sc": b.scalars(),
            "n_syn": b.n_syn()}


def _same_state(got, want, what=""):
    assert got["n_syn"] == want["n_syn"], (what, got["n_syn"], want["n_syn"])
    _same_records(got["syn"], want["syn"], what)
    assert np.array_equal(got["lf"], want["lf"]), what
    assert np.array_equal(got["lv"], want["lv"]), what
    gs, ws = got["sc"], want["sc"]
    assert (gs["clock"], gs["pass_index"]) == (ws["clock"], ws["pass_index"]), (what, gs, ws)
    assert np.array([gs["reward"], gs["rbar"]], F32).tobytes() == np.array([ws["reward"], ws["rbar"]], F32).tobytes(), what


# ---- 1. diff edges --------------------------------------------------------------------------------
@pytest.mark.parametrize("n_syn", SIZES)
def test_diff_record_count_edges(gpu, n_syn):
    then, now = pair(n_syn, n_syn, seed=n_syn + 1)
    with _brain(n_syn) as b:
        b.upload_synapses(then)
        with b.snapshot() as snap:
            info = snap.info()
            assert info["captures"] == 1 and info["n_syn"] == n_syn and info["bytes"] >= 11 * n_syn + 16 * N_NRN
            _diff_equals_reference(snap, then, then, "nothing changed")
            b.upload_synapses(now)
            a0, a1 = b.download_synapses(), None
            _same_records(a0, now)
            res = _diff_equals_reference(snap, then, a0, n_syn)
            if n_syn >= 4095:
                d = res["no range"]
                assert min(d[k] for k in ("dead_both", "killed", "revived", "rewired", "same", "up", "down", "zero", "nan",
                                          "under", "over", "not_summable")) > 0
            # an edit on the device is the other way to B
            head = b.edit("affine", a=1.0, b=0.001953125, dst=(256, 256))
            a1 = b.download_synapses()
            res = _diff_equals_reference(snap, then, a1, (n_syn, "edit"))
            assert res["no range"]["compared"] == n_syn and (head["changed"] == 0 or res["no range"]["changed"] > 0)


# the CPU file's unequal pairs, by the number of tombstones a structural update takes out of 4099 records
assert set(UNEQUAL) == {(4099 - 2, 4099), (4099, 4099 - 3)}


@pytest.mark.parametrize("k", [2, 3], ids=["4099-4097", "4099-4096"])
def test_diff_unequal_sides(gpu, k):
    """n_then != n_now: a structural update shrinks the handle under a snapshot
    (4099 then, 4099 - k now), and a records restore grows it again under a later
    one (4099 - k then, 4099 now).  k = 2 is (4097, 4099): c is odd, so the last
    compared record is in no 16-byte pair and the pair of the longer side that
    holds it goes on with a live record past c; k = 3 is (4099, 4096)."""
    n, m = 4099, 4099 - k
    tombs = [5, 2000, 4090][3 - k:]
    then = records(n, 77)
    then["w"][100:100 + len(SPECIAL_PAIRS)] = SPECIAL_PAIRS[:, 0]
    then["src"][tombs] = NONE  # the update removes them
    then["dst"][tombs] = NONE
    with _brain(n, 256, compact_every=1, w_prune=1e-30) as b:
        b.upload_synapses(then)
        with b.snapshot() as s0:
            b.encode_traversal(1)
            assert b.n_syn() == m and b.structural_updates() == 1
            mid = b.download_synapses()
            res = _diff_equals_reference(s0, then, mid, (n, m))
            assert res["no range"]["gone"] == k and res["no range"]["born"] == 0
            with b.snapshot() as s1:
                assert s1.info()["n_syn"] == m
                _diff_equals_reference(s0, then, mid, (n, m, "two snapshots"), now_snap=s1)
                s0.restore("records")
                assert b.n_syn() == n
                back = b.download_synapses()
                _same_records(back, then)
                assert (back["dst"][m:] != NONE).all()  # live records past c
                res = _diff_equals_reference(s1, mid, back, (m, n))
                assert res["no range"]["born"] == k and res["no range"]["gone"] == 0
                assert b.census(4, 0.0, 1.0)["tombstones"] == k
                # every live weight moves: the paired records below the first hole are changed ones
                b.edit("affine", a=1.0, b=0.001953125)
                moved = b.download_synapses()
                res = _diff_equals_reference(s1, mid, moved, (m, n, "edit"))
                assert res["no range"]["compared"] == m and res["no range"]["changed"] >= max(1, tombs[0] - len(SPECIAL_PAIRS))
                with b.snapshot() as s2:
                    _diff_equals_reference(s1, mid, moved, (m, n, "two snapshots"), now_snap=s2)
                    _diff_equals_reference(s2, moved, mid, (n, m, "the other way"), now_snap=s1)
                b.encode_traversal(1)  # the restored tally feeds the next update
                assert b.n_syn() == m and b.census(4, 0.0, 1.0)["tombstones"] == 0


def test_diff_big_brain_and_contention(gpu):
    import abnn_amd
    from abnn_amd import snapshot

    with abnn_amd.Brain(256, 256, 100_000, BIG, 100_000) as b:
        b.build_random_graph(5)
        then = b.download_synapses()
        with b.snapshot() as snap:
            assert b.edit("affine", a=0.75, b=0.0625, src=(0, 60_000))["changed"] > BIG // 3
            # the last record, in no 16-byte pair: changed whatever its src is
            last = then[BIG - 1]
            b.edit("set", b=float(last["w"]) + 0.25, src=(int(last["src"]), 1), dst=(int(last["dst"]), 1))
            now = b.download_synapses()
            assert now["w"][BIG - 1] != then["w"][BIG - 1]
            for args in ((64, -0.25, 0.25, None, None), (512, -0.5, 0.5, (256, 50_000), (0, 90_000))):
                got = snap.diff(*args[:3], src=args[3], dst=args[4])
                want = snapshot.reference(then, now, snapshot.config(*args))
                invariants(got)
                assert snapshot.to_words(got).tolist() == snapshot.to_words(want).tolist(), args
            assert got["compared"] == BIG and got["changed"] > 0
        # every changed d equal: one LDS address per histogram copy takes every increment
        b.edit("set", b=0.5)
        then = b.download_synapses()
        with b.snapshot() as snap:
            b.edit("set", b=0.75, dst=(0, 60_000))
            now = b.download_synapses()
            for bins in (1, 4096):
                got = snap.diff(bins, -1.0, 1.0)
                want = snapshot.reference(then, now, snapshot.config(bins, -1.0, 1.0))
                assert snapshot.to_words(got).tolist() == snapshot.to_words(want).tolist(), bins
                assert got["changed"] == got["up"] == int(got["counts"].max()) > BIG // 3 and got["max_abs"] == F32(0.25)
                assert got["net"] == got["abs"] == got["changed"] << 22


# ---- 2. two snapshots, the enqueue-only path --------------------------------------------------------
def test_two_snapshots_and_enqueue_on_a_side_stream(gpu):
    import torch

    from abnn_amd import snapshot

    with _learner() as b:
        b.encode_traversal(3)
        side = torch.cuda.Stream(device=0)
        cfg = snapshot.config(256, -0.05, 0.05, dst=(256, 744))
        words = snapshot.n_words(cfg)
        outs = [torch.full((words + 2,), SENTINEL, dtype=torch.int64, device="cuda:0") for _ in range(2)]
        torch.cuda.synchronize()
        from abnn_amd import Snapshot

        with Snapshot(b) as then, Snapshot(b) as now:
            assert then.info()["captures"] == 0
            # captures and diffs between passes, one synchronise at the end
            then.capture(stream=side)
            b.encode_traversal(5, stream=side)
            now.capture(stream=side)
            then.diff_enqueue(cfg, outs[0].data_ptr(), stream=side)
            then.diff_enqueue(cfg, outs[1].data_ptr(), stream=side, now=now)
            b.encode_traversal(2, stream=side)
            side.synchronize()
            assert then.info()["pass_index"] == 3 and now.info()["pass_index"] == 8 and b.scalars()["pass_index"] == 10
            got = [o.cpu().numpy().view(np.uint64) for o in outs]
            assert got[0][-2:].tolist() == [SENTINEL, SENTINEL] and got[0].tolist() == got[1].tolist()
            sync = then.diff(256, -0.05, 0.05, dst=(256, 744), now=now)
            assert snapshot.to_words(sync).tolist() == got[0][:words].tolist() and sync["changed"] > 0
            # the handle has moved on since `now`
            later = then.diff(256, -0.05, 0.05, dst=(256, 744))
            assert later["changed"] > 0 and snapshot.to_words(later).tolist() != got[0][:words].tolist()
            # a twin that ran the same passes, synchronously: the same records at the two captures
            with _learner() as twin:
                twin.encode_traversal(3)
                a = twin.download_synapses()
                twin.encode_traversal(5)
                want = snapshot.reference(a, twin.download_synapses(), cfg)
                assert snapshot.to_words(want).tolist() == got[0][:words].tolist()
            # a second capture overwrites the first
            then.capture()
            b.synchronize()
            assert then.info()["captures"] == 2 and then.diff(8, -1.0, 1.0)["changed"] == 0


# ---- 3. restore equals the state at the capture ------------------------------------------------------
def test_restore_equals_the_state_at_capture(gpu):
    with _learner() as b:
        b.encode_traversal(7)
        with b.snapshot() as snap:
            at = _state(b)
            fired = b.stats()["fired"]
            b.encode_traversal(9)
            assert b.stats()["fired"] > fired and b.budget() < b.params.max_spikes
            d = snap.diff(64, -0.05, 0.05)
            assert d["changed"] > 0 and d["up"] > 0 and d["down"] > 0
            snap.restore()
            _same_state(_state(b), at, "restore")
            assert b.budget() == b.params.max_spikes
            assert snap.diff(64, -0.05, 0.05)["changed"] == 0
            assert b.stats()["passes"] == 16  # the cumulative counters stay


# ---- 4. restore then run equals run -------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(mode=0), dict(mode=1), dict(mode=0, track_visits=1),
                                dict(mode=0, renorm_thresh=10), dict(mode=1, track_visits=1, renorm_thresh=10)],
                         ids=["sweep", "random", "track_visits", "renorm", "random-visits-renorm"])
def test_restore_then_run_equals_run(gpu, kw):
    from abnn_amd import LearnEngine

    rng = np.random.default_rng(3)
    vals = rng.random(256).astype(F32)
    with _learner(**kw) as b:
        b.encode_traversal(7)
        with b.snapshot() as snap:
            renorms = b.renormalisations()
            # hz = 1e-12 makes the firing probability of input i vals[i]: the draw decides
            b.inject_inputs(vals, HZ)
            injected = b.last_fired()
            assert 40 < (injected[:256] == 7).sum() < 216
            b.encode_traversal(P)
            straight = _state(b)
            # anything in between: passes, another draw of the RNG, the device-resident loop
            b.encode_traversal(4)
            b.inject_inputs(vals, 2 * HZ)
            with LearnEngine(b) as eng:
                eng.run(rng.random((3, 256)).astype(F32), rng.random((3, 256)).astype(F32))
                b.synchronize()
            b.encode_traversal(2)
            if "renorm_thresh" in kw:
                assert b.renormalisations() > renorms
            assert b.scalars()["pass_index"] == 7 + P + 9
            snap.restore()
            assert b.scalars()["pass_index"] == 7 and b.scalars()["clock"] == snap.info()["clock"]
            b.inject_inputs(vals, HZ)
            assert np.array_equal(b.last_fired(), injected)
            b.encode_traversal(P)
            _same_state(_state(b), straight, kw)
            # and once more from the same snapshot, without the detour
            snap.restore()
            b.inject_inputs(vals, HZ)
            b.encode_traversal(P)
            _same_state(_state(b), straight, (kw, "again"))


# ---- 5. structural plasticity -------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_restore_with_structural_plasticity(gpu, mode):
    from test_edit_gpu import _readers_agree

    n_syn = 120_000
    with _learner(n_syn, mode=mode, w_prune=0.105, p_new=0.35, w_init=0.5, compact_every=4,
                  syn_capacity=n_syn + 20_000) as b:
        b.encode_traversal(6)  # between the updates after passes 4 and 8
        assert b.structural_updates() == 1
        with b.snapshot() as snap:
            at = _state(b)
            updates = b.structural_updates()
            b.encode_traversal(P)
            straight, d_updates = _state(b), b.structural_updates() - updates
            assert d_updates == 2 and straight["n_syn"] != at["n_syn"]
            b.encode_traversal(5)
            assert b.structural_updates() - updates >= 2 and b.n_syn() != at["n_syn"]
            diff = snap.diff(64, -0.05, 0.05)
            assert diff["n_then"] == at["n_syn"] and diff["n_now"] == b.n_syn() and diff["rewired"] > 0
            updates = b.structural_updates()
            snap.restore()
            got = _state(b)
            _same_state(got, at, "restore")
            _readers_agree(b, got["syn"], "after the restore")
            b.encode_traversal(P)
            _same_state(_state(b), straight, "restore then run")
            assert b.structural_updates() - updates == d_updates
            assert b.census(4, 0.0, 1.0)["records"] == straight["n_syn"]


# ---- 6. parts -----------------------------------------------------------------------------------------
def test_parts(gpu):
    with _learner(track_visits=1) as b:  # so that lastVisited moves too
        b.encode_traversal(5)
        with b.snapshot() as snap:
            at = _state(b)
            b.encode_traversal(6)
            later = _state(b)
            snap.restore("records")  # the timestamps and the scalars stay
            got = _state(b)
            _same_records(got["syn"], at["syn"], "records only")
            assert np.array_equal(got["lf"], later["lf"]) and np.array_equal(got["lv"], later["lv"]) and got["sc"] == later["sc"]
            b.upload_synapses(later["syn"])
            snap.restore(("state",))  # the records stay
            got = _state(b)
            _same_records(got["syn"], later["syn"], "state only")
            assert np.array_equal(got["lf"], at["lf"]) and np.array_equal(got["lv"], at["lv"]) and got["sc"] == at["sc"]
            assert not np.array_equal(at["lv"], later["lv"])  # the plane had moved on
            # records overwritten through the host: the captured ones come back
            junk = later["syn"].copy()
            junk["w"] = F32(0.123)
            junk["dst"][::5] = NONE
            junk["src"][::5] = NONE
            b.upload_synapses(junk)
            snap.restore("records")
            _same_records(b.download_synapses(), at["syn"], "after an upload")
            assert b.census(4, 0.0, 1.0)["tombstones"] == 0
            b.encode_traversal(P)  # records and state are the capture's again: the straight run
            with _learner(track_visits=1) as twin:
                twin.encode_traversal(5 + P)
                _same_state(_state(b), _state(twin), "both parts, one after the other")


# ---- 7. refusals --------------------------------------------------------------------------------------
def test_refusals(gpu):
    import torch

    import abnn_amd
    from abnn_amd import Snapshot, _lib, snapshot

    out = torch.zeros(24 + 4096, dtype=torch.int64, device="cuda:0")
    with _brain(1_000) as b, _brain(1_000) as other:
        b.build_random_graph(1)
        other.build_random_graph(1)
        before = b.checksum()
        good = snapshot.config(8, -1.0, 1.0)
        with Snapshot(b) as empty, b.snapshot() as snap, other.snapshot() as foreign:
            def refused(fn, *args):
                with pytest.raises(abnn_amd.AbnnError) as err:
                    fn(*args)
                assert err.value.status == 1, (fn, args)
                assert b.checksum() == before and b.scalars()["pass_index"] == 0  # the handle stays usable

            refused(empty.restore)                      # nothing captured yet
            refused(empty.diff, 8, -1.0, 1.0)
            refused(snap.diff_enqueue, good, out.data_ptr(), None, empty)
            for what in (0, 4, 7, 0x80000001):          # bad `what`
                refused(_lib.call, "abnn_snapshot_restore", b._h, snap._h, what)
            refused(_lib.call, "abnn_snapshot_restore", b._h, foreign._h, 3)       # a snapshot of another brain
            refused(_lib.call, "abnn_snapshot_capture_enqueue", b._h, foreign._h, None)
            refused(_lib.call, "abnn_snapshot_diff_enqueue", b._h, foreign._h, None, C.byref(good), out.data_ptr(), None)
            refused(_lib.call, "abnn_snapshot_diff_enqueue", b._h, snap._h, foreign._h, C.byref(good), out.data_ptr(), None)
            refused(_lib.call, "abnn_snapshot_diff_enqueue", b._h, snap._h, None, C.byref(good), None, None)
            for bad in (snapshot.config(0, -1.0, 1.0), snapshot.config(4097, -1.0, 1.0), snapshot.config(8, 1.0, 1.0),
                        snapshot.config(8, float("nan"), 1.0), snapshot.config(8, -1.0, 1.0, dst=(990, 11)),
                        snapshot.config(8, -1.0, 1.0, src=(1000, 1))):
                refused(snap.diff_enqueue, bad, out.data_ptr())
                refused(snap.diff, bad.bins, bad.lo, bad.hi, (bad.src_first, bad.src_count), (bad.dst_first, bad.dst_count))
            refused(_lib.call, "abnn_snapshot_diff", b._h, snap._h, None, C.byref(good), out.data_ptr(), 31)  # words
            torch.cuda.synchronize()
            assert not out.cpu().numpy().any()  # a refused diff writes nothing
            assert snap.diff(8, -1.0, 1.0)["same"] == 1_000
            snap.restore()
            b.encode_traversal(2)
            assert b.scalars()["pass_index"] == 2


# ---- 8. shards ----------------------------------------------------------------------------------------
def test_three_shards_equal_the_unsharded_diff(gpu):
    import abnn_amd
    from abnn_amd import snapshot
    from abnn_amd.shard import global_events, shard_ranges

    n_syn, events = 8193, 100_000
    then, now = pair(n_syn, n_syn, seed=31)
    ge = global_events(n_syn, events, 3)
    with _brain(n_syn) as whole:
        whole.upload_synapses(then)
        with whole.snapshot() as snap:
            whole.upload_synapses(now)
            want = _diff_equals_reference(snap, then, now, "unsharded")
    parts = {name: [] for name in CONFIGS}
    for lo, hi in shard_ranges(n_syn, 3):
        with abnn_amd.Brain(256, 256, 488, hi - lo, events, syn_offset=lo, global_events=ge) as s:
            s.upload_synapses(then[lo:hi])
            with s.snapshot() as snap:
                s.upload_synapses(now[lo:hi])
                for name, d in _diff_equals_reference(snap, then[lo:hi], now[lo:hi], (lo, hi)).items():
                    parts[name].append(d)
    for name in CONFIGS:
        merged = snapshot.merge(parts[name])
        assert snapshot.to_words(merged).tolist() == snapshot.to_words(want[name]).tolist(), name
        assert merged["changed"] > 0


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_sharded_brain_snapshot_world1(gpu, monkeypatch):
    import torch.distributed as dist

    from abnn_amd import snapshot
    from abnn_amd.shard import ShardedBrain, TorchComm

    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(_port()))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        sb = ShardedBrain(TorchComm(), 256, 256, 488, 120_000, 120_000, device=0, native=True, seed=13,
                          track_visits=1)
        sb.brain.build_random_graph(21)
        sb.brain.set_auto_stimulus(0, 256)
        sb.step(5)
        snap = sb.snapshot()
        then = sb.brain.download_synapses()
        sb.step(P)
        straight = _state(sb.brain)
        assert sb.brain.stats()["fired"] > 0
        got = sb.diff(snap, 64, -0.05, 0.05, dst=(256, 744))
        want = snapshot.reference(then, straight["syn"], snapshot.config(64, -0.05, 0.05, dst=(256, 744)))
        assert snapshot.to_words(got).tolist() == snapshot.to_words(want).tolist() and got["changed"] > 0
        sb.step(3)
        ge = sb.global_events
        sb.restore(snap)
        assert sb.global_events == ge and sb.brain.scalars()["pass_index"] == 5
        sb.step(P)
        _same_state(_state(sb.brain), straight, "ShardedBrain at world 1")
        snap.close()
        sb.native.close()
        sb.brain.close()
    finally:
        dist.destroy_process_group()


# ---- 9. the C++ mirror --------------------------------------------------------------------------------
def test_cpp_snapshot(gpu):
    from abnn_amd.build import build_snapshot_test

    prog = build_snapshot_test()
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    lines = r.stdout.strip().splitlines()
    assert lines, (r.returncode, r.stderr[-2000:])
    res = json.loads(lines[-1])
    assert r.returncode == 0 and res["ok"], (res, r.stderr[-2000:])
    assert res["records"] == 100_001 and res["changed"] > 0 and res["bytes"] >= 11 * 100_001
