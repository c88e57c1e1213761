"""Scenarios: sequences of record writers and passes, applied to a GPU handle
and to the CPU oracle alike, everything compared on bits after every operation
(tests/test_gpu_scenarios.py), or to the oracle alone (g = None:
tests/test_scenario_model.py, which checks that the scenarios stay busy).

The handle keeps bookkeeping that every writer of the records redoes or drops
(DESIGN.md §9 "Who redoes what"): the structural update's tombstone tally, the
random-mode src mirror, the sweep partition, the src index, the bitmap's
provenance, the grown records, records_invalid.  The per-feature tests pin one
writer at a time against a second GPU handle that got the records through an
upload, which redoes all of it.  Here two or more writers follow each other on
one handle with no upload in between, and the reference is the oracle with the
numpy host rules (edit.reference, reorder.reference / inverse, graph.reference);
no second GPU handle is used anywhere.

An operation is a tuple (name, parameters ...) of plain numbers and strings, so
a failing check can print the operations so far, one per line, and
`replay(kind, seed, upto)` can run that prefix again.  Descriptors whose
parameters depend on the state ("upload_slice" positions, "su_pass") are
resolved against the oracle when they are applied; the log holds what ran.
"""
from __future__ import annotations

import numpy as np

import knob_helpers as K

TOMB = 0xFFFFFFFF
CHUNK = 4096  # kCompactChunk (csrc/engine.h): records per word of the tombstone tally
N_IN = N_OUT = 256

# kind -> ({n_hidden, records, events}, parameters)
KINDS = {
    # 20 000 live records lie past the sweep's end E = 100 096: reorders carry records across it
    "sweep_indexed": ((3000, 120_000, 100_000), {}),
    "sweep_plastic": (K.WIDE, dict(K.SP)),
    "random_plastic": (K.RANDOM_SP, dict(K.SP, mode=1, seed=9, track_visits=1)),
}
INDEXED_ENV = {"ABNN_INDEXED": "2", "ABNN_INDEX_AFTER": "1"}  # sweep_indexed: set before the handle is made

# The ten writers of the ordered pairs; "su_pass" is a pass on which a structural
# update falls (sweep_indexed has none: one more pass, indexed or not by the book).
WRITERS = ("kill_dst", "kill_w", "affine", "reorder_src", "reorder_none", "reorder_random", "restore_records",
           "restore_both", "upload_slice", "su_pass")
# (kind, A, B) combinations that are not legal; none is needed
EXCLUDED = ()
assert len(EXCLUDED) <= 10

# The whole vocabulary, as the walks draw it ("flavour" in the sweep kinds only).
VOCABULARY = ("passes", "reward", "stimulus", "stamp", "flavour", "kill_dst", "kill_src", "kill_w", "affine", "draw",
              "reorder_src", "reorder_dst", "reorder_w", "reorder_none", "reorder_random", "perm", "capture",
              "restore_records", "restore_state", "restore_both", "upload_slice", "build_graph")
RECORD_WRITERS = ("kill_dst", "kill_src", "kill_w", "affine", "draw", "reorder_src", "reorder_dst", "reorder_w",
                  "reorder_none", "reorder_random", "perm", "restore_records", "restore_state", "restore_both",
                  "upload_slice", "build_graph")
# what drops the src index (capi.hip index_invalidate's callers); AFFINE and DRAW write weights only,
# a restore of the state alone writes no record
INVALIDATES = ("kill_dst", "kill_src", "kill_w", "reorder_src", "reorder_dst", "reorder_w", "reorder_none",
               "reorder_random", "perm", "restore_records", "restore_both", "upload_slice", "build_graph")
# chosen on the CPU (tests/test_scenario_model.py holds the conditions they meet)
WALK_SEEDS = {
    "sweep_indexed": (0, 1, 8, 11, 12, 23),
    "sweep_plastic": (0, 1, 8, 11, 13, 23),
    "random_plastic": (4, 8, 9, 14, 18, 34),
}
WALK_OPS = 40


class ScenarioFailure(AssertionError):
    pass


def _tombs(syn):
    return int(np.count_nonzero(syn["src"] == TOMB))


class Scenario:
    """One handle (or none) and one oracle of a kind, and the test's own book
    of what the handle's bookkeeping should say."""

    def __init__(self, kind, seed=None, gpu=True):
        self.kind, self.seed = kind, seed
        self.shape, self.params = KINDS[kind]
        self.g, self.o = K.pair(self.shape, K.graph(self.shape), gpu=gpu, **self.params)
        self.n_nrn = self.o.n_neuron()
        self.ce = int(self.params.get("compact_every", 0))
        self.mode = int(self.params.get("mode", 0))
        self.ops, self.log, self.skipped = [], [], 0
        self.snaps, self.gsnaps = {}, {}
        self.origin = None  # the last origin a reorder returned
        self.su = 0  # structural updates so far
        self.fused = True
        self.ix_built, self.ix_eligible, self.last_indexed = False, 0, False  # the src index's book
        self.killed_chunks = set()  # chunks in which a KILL tallied tombstones that are still there
        self.reordered = False  # a reorder ran and no structural update (indexed pass) since
        self._stats = (self.g.stats() if gpu else None, self.o.stats())

    def close(self):
        for s in self.gsnaps.values():
            s.close()
        self.gsnaps = {}
        if self.g is not None:
            self.g.close()
            self.g = None

    # ---- resolving a descriptor against the state; None: not legal now -------------------------
    def resolve(self, d):
        name, n = d[0], int(self.o.s.dims.n_syn)
        if name == "su_pass":  # the passes up to and with the next structural update
            return ("passes", self.ce - int(self.o.s.pass_index) % self.ce if self.ce else 1)
        if name == "flavour" and self.mode != 0:
            return None  # the sweep kinds only
        if name.startswith("restore") and d[1] not in self.snaps:
            return None
        if name == "perm" and (self.origin is None or len(self.origin) != n):
            return None
        if name == "upload_slice" and isinstance(d[1], str):
            where, step = d[1], d[2]
            if where == "cross":  # across a chunk boundary among the sparse records (past the dense 65 536)
                first, cnt = (n * 3 // 4 // CHUNK) * CHUNK - 700, 1500
            elif where == "last":  # inside the last chunk
                first = (n - 1) // CHUNK * CHUNK
                first, cnt = first + (n - first) // 4, max(1, (n - first) // 2)
            else:  # across m = n_syn - D, the boundary of the O(D) fill
                m = n - _tombs(self.o.syn)
                first, cnt = max(0, m - 300), 600
            return ("upload_slice", int(first), int(min(cnt, n - first)), int(step))
        return d

    # ---- one operation -------------------------------------------------------------------------
    def apply(self, d):
        """Resolves and runs a descriptor on the handle and the oracle, then
        compares.  False: the draw was not legal in this state (counted)."""
        op = self.resolve(d)
        if op is None:
            self.skipped += 1
            return False
        self.ops.append(op)
        try:
            entry = getattr(self, "_" + op[0].split("_")[0])(*op)
            entry.update(op=op, name=d[0] if d[0] == "su_pass" else op[0])
            self._book(entry)
            self._check(entry)
        except ScenarioFailure:
            raise
        except Exception as e:  # an assertion, or an error of the library
            raise ScenarioFailure(f"{type(e).__name__}: {e}\n{self.describe()}") from e
        self.log.append(entry)
        return True

    def describe(self):
        lines = "\n".join(f"  {i}: {op!r}" for i, op in enumerate(self.ops))
        return (f"kind {self.kind!r}, seed {self.seed!r}, after {len(self.ops)} operations (the last one failed; "
                f"scenario_helpers.replay(kind, seed, upto) runs a prefix again):\n{lines}")

    # passes and state
    def _passes(self, _, k):
        o, su0, n0 = self.o, self.su, int(self.o.s.dims.n_syn)
        if self.g is not None:
            self.g.encode_traversal(k)
        indexed, changed_n = [], False
        for _ in range(k):
            o.pass_serial(1)
            if self.ce and int(o.s.pass_index) % self.ce == 0:
                self.su += 1
                self.killed_chunks.clear()
            # the index's book (capi.hip run_fused / run_gate): built in front of a fused pass once one
            # eligible pass has run since the index was dropped; a two-kernel pass is not an eligible one
            if self.kind == "sweep_indexed" and self.fused:
                self.ix_built = self.ix_built or self.ix_eligible >= 1
                self.ix_eligible += 1
                indexed.append(self.ix_built)
            else:
                self.ix_eligible = 0
                indexed.append(False)
            changed_n = changed_n or int(o.s.dims.n_syn) != n0
        self.last_indexed = indexed[-1]
        su_last = bool(self.ce) and int(o.s.pass_index) % self.ce == 0
        if su_last:
            assert _tombs(o.syn) == 0, "tombstones straight after a structural update"
        return dict(passes=k, su=self.su - su0, su_last=su_last, indexed=indexed, n_changed=changed_n,
                    after_reorder=self.reordered and (self.su > su0 or any(indexed)))

    def _reward(self, _, r):
        for x in self._both():
            x.set_reward(r)
        return {}

    def _stimulus(self, _, first, count):
        for x in self._both():
            x.set_auto_stimulus(first, count)
        return {}

    def _stamp(self, _, idx, d):
        value = int(self.o.s.clock) + d  # d = 2: ahead of the clock
        for x in self._both():
            x.set_timestamps(list(idx), value)
        return {}

    def _flavour(self, _, which):
        self.fused = which == "fused"
        if self.g is not None:
            assert self.g._lib.abnn_debug_set_fused(self.g._h, int(self.fused)) == 0
        return {}

    # record writers
    def _edit(self, op, **kw):
        from abnn_amd import edit

        o = self.o
        new, head = edit.reference(o.syn, edit.config(op, **kw), self.n_nrn)
        was = o.syn.copy()
        o.set_synapses(new)
        if self.g is not None:
            got = self.g.edit(op, **kw)
            assert got == head, f"edit header {got} != {head}"
        if op == "kill":
            self.killed_chunks.update(np.unique(np.flatnonzero(was["src"] != new["src"]) // CHUNK).tolist())
        return dict(killed=head["killed"], changed=head["changed"])

    def _kill(self, name, *p):
        by = name.split("_")[1]
        if by == "w":
            return self._edit("kill", weights=(p[0], p[1]))
        return self._edit("kill", **{by: (p[0], p[1])})

    def _affine(self, _, w_lo, w_hi, a, b, c_lo, c_hi):
        return self._edit("affine", weights=(w_lo, w_hi), a=a, b=b, clamp=(c_lo, c_hi))

    def _draw(self, _, first, count, a, b, seed):
        return self._edit("draw", src=(first, count), a=a, b=b, seed=seed)

    def _reorder(self, name, descending=False, seed=0, perm=None):
        from abnn_amd import reorder

        o, key = self.o, name.split("_")[1] if perm is None else "perm"
        tomb = _tombs(o.syn)
        new, origin, head = reorder.reference(o.syn, reorder.config(key, bool(descending), seed, True), perm=perm)
        o.set_synapses(new)
        if self.g is not None:
            got = self.g.reorder(None if perm is not None else key, bool(descending), seed, origin=True, perm=perm)
            assert np.array_equal(got.pop("origin"), origin), "the reorder's origin"
            assert got == head, f"reorder header {got} != {head}"
        assert head["invalid"] == 0
        self.origin = origin
        self.killed_chunks = set(range((len(new) - tomb) // CHUNK, (len(new) + CHUNK - 1) // CHUNK)) if tomb and self.killed_chunks else set()
        self.reordered = True
        return dict(moved=head["moved"], tombstones=tomb)

    def _perm(self, _):
        from abnn_amd import reorder

        return self._reorder("reorder_perm", perm=reorder.inverse(self.origin))

    def _capture(self, _, slot):
        o = self.o
        self.snaps[slot] = dict(n=int(o.s.dims.n_syn), syn=o.syn.copy(), lf=o.last_fired.copy(), lv=o.last_visited.copy(),
                                grown=o._grown.copy(),
                                scalars={k: getattr(o.s, k) for k in ("clock", "reward", "rbar", "rng", "pass_index")})
        if self.g is not None:
            if slot not in self.gsnaps:
                self.gsnaps[slot] = self.g.snapshot()
            else:
                self.gsnaps[slot].capture()
                self.g.synchronize()
        return {}

    def _restore(self, name, slot):
        """abnn_snapshot_restore (capi.hip): RECORDS brings back records [0, n)
        and n_syn; STATE the two timestamp arrays, the scalar block {clock,
        reward, rbar, pass_index}, the inject_inputs RNG and the grown records.
        The cumulative statistics, the stimulus range and the count of
        structural updates stay the handle's."""
        o, s, what = self.o, self.snaps[slot], name.split("_")[1]
        entry = dict(n_before=int(o.s.dims.n_syn), n_after=int(o.s.dims.n_syn))
        if what in ("records", "both"):
            entry["differs"] = s["n"] != len(o.syn) or o.syn.tobytes() != s["syn"].tobytes()
            entry["n_after"] = s["n"]
            o.set_synapses(s["syn"])
            o.s.dims.n_syn = s["n"]
            self.killed_chunks.clear()
        if what in ("state", "both"):
            o.last_fired[:] = s["lf"]
            o.last_visited[:] = s["lv"]
            o._grown[:] = s["grown"]
            for k, v in s["scalars"].items():
                setattr(o.s, k, v)
        if self.g is not None:
            self.gsnaps[slot].restore({"records": ("records",), "state": ("state",), "both": ("records", "state")}[what])
        return entry

    def _upload(self, _, first, n, step):
        """A partial upload of the oracle's current records [first, first + n)
        with every step-th one made a tombstone."""
        o = self.o
        part = o.syn[first:first + n].copy()
        part["pad"] = 0.0
        at = np.arange(step // 2, n, step)
        part["src"][at] = TOMB
        part["dst"][at] = TOMB
        chunks = set(range(first // CHUNK, (first + n - 1) // CHUNK + 1))
        entry = dict(over_killed=bool(chunks & self.killed_chunks), planted=int(at.size), first=first, n=n)
        o._syn[first:first + n] = part
        if self.g is not None:
            self.g.upload_synapses(part, first)
        return entry

    def _build(self, _, seed):
        from abnn_amd import graph

        o, n = self.o, int(self.o.s.dims.n_syn)
        spec = graph.recipe(N_IN, N_OUT, self.shape[0], n, seed)
        o.set_synapses(graph.reference(spec, 0, n))
        if self.g is not None:
            self.g.build_graph(spec)
        self.killed_chunks.clear()
        return {}

    # ---- the book and the checks ---------------------------------------------------------------
    def _both(self):
        return [x for x in (self.g, self.o) if x is not None]

    def _book(self, entry):
        if entry["op"][0] in INVALIDATES:
            self.ix_built, self.ix_eligible = False, 0
        if entry.get("after_reorder"):
            self.reordered = False

    def _check(self, entry):
        g, o, what = self.g, self.o, f"after {entry['op']!r}"
        so = o.stats()
        entry["stats"] = {k: so[k] - self._stats[1][k] for k in so}
        entry["n_syn"], entry["tombstones"] = int(o.s.dims.n_syn), _tombs(o.syn)
        if g is None:
            self._stats = (None, so)
            return
        K.same(g, o, what)
        sg = g.stats()
        assert {k: sg[k] - self._stats[0][k] for k in sg} == entry["stats"], f"statistics {what}: {sg} != {so}"
        self._stats = (sg, so)
        if self.params.get("track_visits"):
            assert np.array_equal(g.last_visited(), o.last_visited), f"lastVisited {what}"
        from oracle import oracle as O

        assert g.visited_events() == O.visited_events(self.shape[2], entry["n_syn"], self.mode), f"visited events {what}"
        assert g.structural_updates() == self.su, f"structural updates {what}: {g.structural_updates()} != {self.su}"
        assert g.census(8, -0.5, 1.5)["tombstones"] == entry["tombstones"], f"the census's tombstones {what}"
        if self.kind == "sweep_indexed":
            from test_gpu_indexed import index_state, mask_dirty

            st = index_state(g)
            assert bool(st["built"]) == self.ix_built, f"the index {what}: {st}, the book says built = {self.ix_built}"
            if entry["op"][0] == "passes":
                assert bool(st["last_indexed"]) == self.last_indexed, f"{what}: {st}, the book says {entry['indexed']}"
                assert mask_dirty(g) == 0, f"the event mask is not clean {what}"
        if entry["op"][0] in RECORD_WRITERS:
            from test_edit_gpu import _readers_agree

            _readers_agree(g, o.syn, what)


def run(scn, descs, upto=None):
    for d in descs[:upto]:
        scn.apply(d)
    return scn


# ---- a. ordered pairs ---------------------------------------------------------------------------
def writer(kind, name, second):
    """The descriptor of pair writer `name`, as A (second = False) or as B: the
    ranges, bands, orders and slots differ, so that B changes something after
    an A of the same name."""
    assert kind in KINDS
    return {
        "kill_dst": ("kill_dst", 1000 if second else 600, 300),
        "kill_w": ("kill_w", 0.15, 0.155) if second else ("kill_w", 0.12, 0.125),
        "affine": ("affine", 0.13, 0.17, 1.1, -0.01, 0.11, 0.18),
        "reorder_src": ("reorder_src", int(second)),  # B: descending
        "reorder_none": ("reorder_none",),
        "reorder_random": ("reorder_random", 0, 5 + int(second)),
        # B restores slot 1, captured one pass after slot 0 (pair_ops)
        "restore_records": ("restore_records", int(second)),
        "restore_both": ("restore_both", int(second)),
        "upload_slice": ("upload_slice", "m" if second else "cross", 7),
        "su_pass": ("su_pass",),
    }[name]


def pair_ops(kind, a, b):
    """The issue's sequence: three passes, capture, two passes, A, B, passes
    until a structural update has run and two more (sweep_indexed: four
    passes, one by one).  Between the two passes slot 1 is captured as well: a
    restore as B takes that one, so that it differs from what a restore as A
    (slot 0) left (the first three passes from lastFired = 0 update no weight,
    so a capture of the fresh pair would equal slot 0)."""
    assert (kind, a, b) not in EXCLUDED
    head = [("passes", 3), ("capture", 0), ("passes", 1), ("capture", 1), ("passes", 1), writer(kind, a, False),
            writer(kind, b, True)]
    tail = [("passes", 1)] * 4 if kind == "sweep_indexed" else [("su_pass",), ("passes", 2)]
    return head + tail


PAIR_HEAD = 7  # operations of pair_ops up to and with B


def run_pair(kind, a, b, gpu=True, upto=None):
    scn = Scenario(kind, ("pair", a, b), gpu)
    try:
        return run(scn, pair_ops(kind, a, b), upto)
    finally:
        scn.close()


# ---- b. seeded walks ----------------------------------------------------------------------------
def draw(rng, kind):
    """One draw from the vocabulary: passes at a third, the rest alike."""
    n_nrn = 512 + KINDS[kind][0][0]
    names = [v for v in VOCABULARY[1:] if v != "flavour" or KINDS[kind][1].get("mode", 0) == 0]
    name = "passes" if rng.random() < 1 / 3 else names[int(rng.integers(len(names)))]
    u, i = (lambda lo, hi: round(float(rng.uniform(lo, hi)), 4)), (lambda lo, hi: int(rng.integers(lo, hi)))
    if name == "passes":
        return (name, i(1, 4))
    if name == "reward":
        return (name, (0.5, -3.0, 0.0, 1.0)[i(0, 4)])
    if name == "stimulus":
        return (name,) + ((0, 256), (0, 0), (32, 200), (100, 156), (255, 1), (64, 100))[i(0, 6)]
    if name == "stamp":
        return (name, tuple(i(0, n_nrn) for _ in range(5)), (0, 2)[i(0, 2)])
    if name == "flavour":
        return (name, ("fused", "two_kernel")[i(0, 2)])
    if name == "kill_dst":
        return (name, i(256, n_nrn - 200), i(20, 200))
    if name == "kill_src":  # the outputs have no outgoing record: inputs or hidden neurons
        return (name, 0, i(5, 60)) if i(0, 4) == 0 else (name, i(512, n_nrn - 200), i(20, 200))
    if name == "kill_w":
        lo = u(0.1, 0.19)
        return (name, lo, round(lo + 0.004, 4))
    if name == "affine":
        lo = u(0.1, 0.6)
        return (name, lo, round(lo + 0.1, 4), u(0.8, 1.2), u(-0.02, 0.02), 0.05, 0.9)
    if name == "draw":
        return (name, i(512, n_nrn - 300), i(20, 300), 0.11, 0.3, i(1, 2**31))
    if name in ("reorder_src", "reorder_dst", "reorder_w"):
        return (name, i(0, 2))
    if name == "reorder_random":
        return (name, 0, i(1, 2**31))
    if name in ("capture", "restore_records", "restore_state", "restore_both"):
        return (name, i(0, 2))
    if name == "upload_slice":
        return (name, ("cross", "last", "m")[i(0, 3)], (3, 7, 50)[i(0, 3)])
    if name == "build_graph":
        return (name, i(1, 2**31))
    return (name,)  # reorder_none, perm


def run_walk(kind, seed, gpu=True, upto=None, n_ops=WALK_OPS):
    """n_ops draws of numpy.random.default_rng(seed); a draw that is not legal
    in the current state is skipped and counted (Scenario.skipped)."""
    rng = np.random.default_rng(seed)
    scn = Scenario(kind, seed, gpu)
    try:
        for _ in range(n_ops):
            d = draw(rng, kind)
            if upto is not None and len(scn.ops) >= upto:
                break
            scn.apply(d)
        return scn
    finally:
        scn.close()


# ---- c. named sequences -------------------------------------------------------------------------
NAMED = {
    # KILL, reorder, KILL again, then a structural update
    "kill_reorder_kill_update": (("sweep_plastic", "random_plastic"), [
        ("passes", 3), ("kill_dst", 600, 300), ("reorder_src", 0), ("kill_w", 0.12, 0.125), ("su_pass",), ("passes", 2)]),
    # a records-only restore onto a handle whose n_syn has changed and whose grown list is half full
    "records_restore_onto_grown_half_full": (("sweep_plastic", "random_plastic"), [
        ("passes", 2), ("capture", 0), ("passes", 3), ("restore_records", 0), ("su_pass",), ("passes", 2)]),
    # a partial upload over chunks that a KILL had tallied
    "upload_over_killed_chunks": (("sweep_plastic", "random_plastic"), [
        ("passes", 3), ("kill_dst", 600, 300), ("upload_slice", "cross", 7), ("upload_slice", "last", 3),
        ("upload_slice", "m", 7), ("su_pass",), ("passes", 2)]),
    # a reorder that carries records across the sweep's end E while an index over [0, E) exists
    "reorder_across_the_sweep_end": (("sweep_indexed",), [
        ("passes", 3), ("reorder_random", 0, 3), ("passes", 2), ("kill_dst", 600, 300), ("reorder_src", 0), ("passes", 2),
        ("perm",), ("passes", 2)]),
    # a restore of the state only, followed by an indexed pass: six passes after the capture, so that the
    # pass before the restore has built the next bitmap from the spike lists (window_pre = 5 clean passes)
    # and the restore has a provenance to drop
    "state_restore_then_indexed_pass": (("sweep_indexed",), [
        ("passes", 3), ("capture", 0), ("passes", 6), ("restore_state", 0), ("passes", 1), ("passes", 2)]),
}


def run_named(name, kind, gpu=True, upto=None):
    scn = Scenario(kind, name, gpu)
    try:
        return run(scn, NAMED[name][1], upto)
    finally:
        scn.close()


def replay(kind, seed, upto, gpu=True):
    """The first `upto` operations of a scenario again: `seed` is a walk's
    seed, ("pair", A, B), or a named sequence's name."""
    if isinstance(seed, str):
        return run_named(seed, kind, gpu, upto)
    if isinstance(seed, tuple):
        return run_pair(kind, seed[1], seed[2], gpu, upto)
    return run_walk(kind, seed, gpu, upto)
