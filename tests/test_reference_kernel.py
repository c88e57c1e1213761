"""The oracle against the reference kernel's own text (CPU).

`oracle/c1_oracle.c` is this project's restatement of the reference's kernel
file; every GPU parity test ends at it.  Here it is compared with that file
itself, compiled in place as host C++ behind a stand-in metal_stdlib and run
under schedule C1 (oracle/ref_recipe/):

* a live differential on the cases of tests/ref_kernel_helpers.py: every word
  after every pass (records, lastF mod 2^32, clock mod 2^32, budget left,
  rBar's bits);
* a seeded fuzz of tiny cases around the edges of the grid, the clock, the
  budget and the weights;
* the fixtures tests/golden/ref_case*.json, made from `ref_pass`
  (tests/golden/make_ref_golden.py): the oracle reproduces them (runs
  everywhere, needs no oracle/_ref/), and regenerating them from the compiled
  reference gives the committed bytes (so they cannot quietly become oracle
  outputs).

The live tests skip only where there is neither a reference checkout nor an
oracle/_ref/ from an earlier build; with a checkout a failed build fails."""
import numpy as np
import pytest

import knob_helpers as K
import ref_kernel_helpers as R

needs_ref = pytest.mark.skipif(not R.ref_available(),
                               reason="no reference checkout (ABNN_REFERENCE_DIR) and no oracle/_ref/ to load")
_BUSY = {}  # case -> the oracle's statistics of its runs so far
RUNS = [(name, i) for name, c in R.CASES.items() for i in range(len(c["runs"]))]


def _differential(ref, orc, passes, reward_from, what):
    d = R.first_difference(orc.observe(), ref.observe())
    assert d is None, f"{what} before pass 0: {d}"
    for k in range(passes):
        if reward_from is not None and k == reward_from:
            ref.set_reward(0.5)
            orc.set_reward(0.5)
        ref.step()
        orc.step()
        d = R.first_difference(orc.observe(), ref.observe())
        assert d is None, f"{what} pass {k}, oracle against reference: {d}"


# ---- the cases, live ----------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("name,run", RUNS, ids=[f"{n}-{i}" for n, i in RUNS])
def test_oracle_equals_reference_kernel_every_pass(name, run):
    ref, s = R.case_runner(R.RefRunner, name, run)
    orc, _ = R.case_runner(R.OracleRunner, name, run)
    _differential(ref, orc, R.CASES[name]["passes"], s["reward_from"], f"{name} run {run}")
    st = orc.o.stats()
    _BUSY.setdefault(name, []).append(st)
    if (name, run) not in R.EXEMPT_FROM_BUSY:
        assert st["fired"] > 0 and st["updated"] >= st["fired"], st
    if len(_BUSY[name]) == len(R.CASES[name]["runs"]):  # the case as a whole: its runs together
        fired, updated = (sum(x[k] for x in _BUSY[name]) for k in ("fired", "updated"))
        assert fired > 0 and updated > fired, (name, fired, updated)
    if s["renorm_thresh"] != R.NEVER:
        assert orc.o.renormalisations() == 1
    if s["special"]:  # every special class is still among the weights the passes read
        assert all(m.any() for m in K.weight_classes(R.case_graph(R.CASES[name]["shape"], True)["w"]).values())


# ---- the fuzz -----------------------------------------------------------------------------------
FUZZ = 240
BUDGETS = (0, 1, 2, 17, 2560, 2**32 - 1)


def fuzz_case(seed):
    """A tiny case from numpy's default_rng(seed).  Every src and dst is a
    neuron and no record is a tombstone: the reference kernel indexes lastF
    unchecked."""
    from oracle import oracle as O

    g = np.random.default_rng(seed)
    n_nrn = int(g.integers(20, 601))
    kind = seed % 6  # the size of the array against the 256-thread groups
    if kind == 0:
        n_syn = int(g.integers(1, 12))
    elif kind == 1:
        n_syn = 256 * int(g.integers(1, 12)) + int(g.integers(-1, 2))
    else:
        n_syn = int(g.integers(1, 3001))
    n_syn = min(max(n_syn, 1), 3000)
    ev_kind = (seed // 6) % 7  # events against n_syn and the groups
    events = {0: int(g.integers(1, n_syn + 1)), 1: n_syn, 2: n_syn + int(g.integers(1, n_syn + 1)), 3: 2 * n_syn, 4: 1,
              5: 256 * int(g.integers(1, 2 * n_syn // 256 + 2)) + int(g.integers(-1, 2)),
              6: max(1, n_syn - 1)}[ev_kind]
    events = min(max(events, 1), 2 * n_syn)
    ck = g.integers(0, 4)  # the clock: small, anywhere, within 8 of 2^32
    clock0 = int(g.integers(0, 10)) if ck == 0 else 2**32 - int(g.integers(1, 9)) if ck == 1 else int(g.integers(0, 2**32))
    # stamps: recent, equal to the clock, ahead of it, anywhere, zero
    how = g.integers(0, 5, n_nrn)
    lastF = np.where(how == 0, clock0 - g.integers(1, 9, n_nrn),
                     np.where(how == 1, clock0, np.where(how == 2, clock0 + g.integers(1, 4, n_nrn),
                                                         np.where(how == 3, g.integers(0, 2**32, n_nrn), 0))))
    lastF = (lastF & R.U32).astype(np.uint32)
    syn = np.zeros(n_syn, dtype=O.SYN_DTYPE)
    syn["src"] = g.integers(0, n_nrn, n_syn)
    syn["dst"] = g.integers(0, n_nrn, n_syn)
    syn["w"] = g.random(n_syn, dtype=np.float32)
    special = seed % 4 == 3
    if special:  # 5 % special values
        at = np.flatnonzero(g.random(n_syn) < 0.05)
        syn["w"].view(np.uint32)[at] = K.SPECIAL_BITS[g.integers(0, K.SPECIAL_BITS.size, at.size)]
    renorm = seed % 5 == 4 and clock0 < 2**32 - 16  # the host renormalises after the third pass
    return dict(syn=syn, n_nrn=n_nrn, events=events, passes=int(g.integers(3, 7)), clock0=clock0, lastF=lastF,
                max_spikes=BUDGETS[int(g.integers(0, len(BUDGETS)))], reward=float(g.uniform(-1.0, 1.0)),
                stim=int(g.integers(0, min(n_nrn, 16) + 1)), special=special,
                renorm_thresh=clock0 + 1 if renorm else R.NEVER)


def _fuzz_runners(c):
    kw = dict(max_spikes=c["max_spikes"], clock0=c["clock0"], renorm_thresh=c["renorm_thresh"], stim=c["stim"],
              last_fired0=c["lastF"], reward=c["reward"])
    return (R.RefRunner(c["syn"], c["n_nrn"], c["events"], **kw),
            R.OracleRunner(c["syn"], c["n_nrn"], c["events"], dims=(4, 4), **kw))


def test_fuzz_covers_its_edges():
    """The generator reaches what it is there for (no reference needed)."""
    cs = [fuzz_case(s) for s in range(FUZZ)]
    n, e = np.array([len(c["syn"]) for c in cs]), np.array([c["events"] for c in cs])
    assert n.min() >= 1 and n.max() <= 3000 and (e >= 1).all() and (e <= 2 * n).all()
    assert (e < n).any() and (e == n).any() and (e > n).any() and (e == 2 * n).any()
    for x in (n, e):  # one below, at and one above a multiple of the group size
        assert {255, 0, 1} <= set((x[x >= 255] % 256).tolist())
    assert {c["max_spikes"] for c in cs} == set(BUDGETS)
    assert any(c["clock0"] >= 2**32 - 8 for c in cs) and any(c["clock0"] < 10 for c in cs)
    assert any(c["clock0"] + c["passes"] > 2**32 for c in cs)  # the clock wraps inside a run
    assert {c["passes"] for c in cs} == {3, 4, 5, 6}
    assert min(c["n_nrn"] for c in cs) < 60 and max(c["n_nrn"] for c in cs) > 500
    assert 0.2 < np.mean([c["special"] for c in cs]) < 0.3
    assert sum(c["renorm_thresh"] != R.NEVER for c in cs) >= 20
    assert all((c["syn"]["src"] < c["n_nrn"]).all() and (c["syn"]["dst"] < c["n_nrn"]).all() for c in cs)
    ahead = [((c["lastF"].astype(np.int64) - c["clock0"]) & R.U32) for c in cs]
    assert all(((a >= 1) & (a <= 3)).any() and (a == 0).any() for a in ahead)


@needs_ref
def test_fuzz_oracle_equals_reference_kernel():
    fired = updated = renorms = 0
    for seed in range(FUZZ):
        c = fuzz_case(seed)
        ref, orc = _fuzz_runners(c)
        _differential(ref, orc, c["passes"], None, f"fuzz seed {seed} ({len(c['syn'])} records, {c['events']} events, "
                      f"budget {c['max_spikes']}, clock {c['clock0']})")
        st = orc.o.stats()
        fired, updated, renorms = fired + st["fired"], updated + st["updated"], renorms + orc.o.renormalisations()
    assert fired > 1000 and updated > 4 * fired and renorms >= 20, (fired, updated, renorms)


# ---- the fixtures -------------------------------------------------------------------------------
def test_reference_fixtures_present():
    import os

    assert all(os.path.exists(R.fixture_path(name)) for name in R.CASES)
    largest = max(os.path.getsize(os.path.join(R.GOLDEN, f)) for f in os.listdir(R.GOLDEN)
                  if f.endswith(".json") and not f.startswith("ref_"))
    assert all(os.path.getsize(R.fixture_path(name)) <= largest for name in R.CASES)


@pytest.mark.parametrize("name", list(R.CASES))
def test_oracle_reproduces_reference_fixture(name):
    g = R.load_fixture(name)
    c = R.CASES[name]
    assert (g["n_hidden"], g["n_syn"], g["events"]) == tuple(c["shape"]) and len(g["runs"]) == len(c["runs"])
    for i, run in enumerate(g["runs"]):
        assert R.fixture_settings(run) == R.run_settings(c["runs"][i]) and len(run["passes"]) == c["passes"]
        orc, _ = R.case_runner(R.OracleRunner, name, i)
        R.check_against_fixture(orc, run, f"oracle, {name} run {i}")
    # the fixture's own counts say the case was busy (a budget of 1 ends a pass's updates at its first
    # spike, so a single run may change no more records than it fires: the case's runs count together)
    fired = [sum(run["max_spikes"] - p["budget_left"] for p in run["passes"]) for run in g["runs"]]
    changed = [sum(p["changed_records"] for p in run["passes"]) for run in g["runs"]]
    assert all(f > 0 for i, f in enumerate(fired) if (name, i) not in R.EXEMPT_FROM_BUSY)
    assert sum(changed) > sum(fired), (fired, changed)


@needs_ref
@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_fixture_regenerates_to_the_committed_bytes(name):
    with open(R.fixture_path(name)) as f:
        committed = f.read()
    assert R.fixture_text(R.case_fixture(R.RefRunner, name)) == committed
