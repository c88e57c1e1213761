"""Off the default knobs on the CPU alone (tests/knob_helpers.py): the oracle
against the Python restatement of brain.metal for every knob and weight case,
its threaded pass and shard phases against its serial pass, and the
conditions that make tests/test_gpu_knobs.py meaningful, asserted on the
oracle at the GPU tests' own shapes.  A case whose knobs let nothing fire, or
whose special weights never reached the update, would let those tests pass
while proving nothing."""
import functools

import numpy as np
import pytest

import knob_helpers as K
from py_reference import MetalEmu, metal_clamp
from shard_helpers import oracle_shard_pass
from test_oracle import _emu_from

F = np.float32
ALL_CASES = [("knob", k) for k in K.KNOBS] + [("weights", k) for k in K.WEIGHT_CASES]
IDS = [f"{a}:{b}" for a, b in ALL_CASES]


def _case(kind, name):
    """(knobs, reward schedule, special weights?) of a case."""
    if kind == "knob":
        return K.KNOBS[name][0], K.KNOBS[name][1], False
    return K.WEIGHT_CASES[name], K.REWARDS, True


# ---- a. Metal's clamp -------------------------------------------------------------------------
def test_metal_clamp_is_fmin_of_fmax():
    """clamp(x, lo, hi) = fmin(fmax(x, lo), hi) (Metal): a NaN x gives lo, as
    csrc/device.h clampf and the C oracle's; signed zeros and payloads pass
    through a select untouched."""
    nan, inf = F(np.nan), F(np.inf)
    assert metal_clamp(nan, F(0.001), F(1.0)) == F(0.001)
    assert metal_clamp(nan, F(0.3), F(0.2)) == F(0.2)  # crossed bounds: min(lo, hi)
    assert metal_clamp(nan, F(0.0), inf) == 0 and not np.signbit(metal_clamp(nan, F(0.0), inf))
    assert metal_clamp(inf, F(0.0), F(2.0)) == F(2.0) and metal_clamp(-inf, F(-1.0), F(1.0)) == F(-1.0)
    assert metal_clamp(F(0.5), F(0.3), F(0.2)) == F(0.2) and metal_clamp(F(0.1), F(0.3), F(0.2)) == F(0.2)
    assert not np.signbit(metal_clamp(F(-0.0), F(0.0), F(1.0)))  # -0 > +0 is false: lo, which is +0
    assert np.signbit(metal_clamp(F(-0.0), F(-1.0), F(1.0)))
    tiny = F(1e-40)
    assert metal_clamp(tiny, F(0.0), inf).view(np.uint32) == tiny.view(np.uint32)  # no flush


def test_special_weights_layout():
    syn = K.graph(K.SMALL)
    before = syn["w"].copy()
    got = K.special_weights(syn)
    assert got is syn
    bits = syn["w"].view(np.uint32)
    assert np.array_equal(bits[0:3 * 14:3], K.SPECIAL_BITS) and np.array_equal(bits[42:84:3], K.SPECIAL_BITS)
    keep = np.arange(len(syn)) % 3 != 0
    assert np.array_equal(syn["w"][keep], before[keep])
    assert [bool(m.any()) for m in K.weight_classes(syn["w"]).values()] == [True] * 6
    assert K.f32_bits(syn["w"][3]) == 0xFFC00001 and K.f32_bits(syn["w"][15]) == 0x80000000


# ---- b. the oracle against the restatement, its other passes against the serial one -----------
def _same_as_emu(ob, emu, what):
    assert ob.clock == emu.clock, what
    assert np.array_equal(ob.last_fired, np.array(emu.lastF, dtype=np.uint64)), what
    assert int(ob.s.dims.n_syn) == len(emu.src), what
    assert np.array_equal(ob.syn["src"], np.array(emu.src, dtype=np.uint32)), what
    assert np.array_equal(ob.syn["dst"], np.array(emu.dst, dtype=np.uint32)), what
    w = np.array(emu.w, dtype=np.float32)
    differ = np.flatnonzero(ob.syn["w"].view(np.uint32) != w.view(np.uint32))
    assert differ.size == 0, (what, differ[:5], ob.syn["w"][differ[:5]], w[differ[:5]])
    assert K.f32_bits(ob.s.rbar) == K.f32_bits(emu.rbar), what


@pytest.mark.parametrize("kind,name", ALL_CASES, ids=IDS)
def test_serial_oracle_matches_python_restatement(kind, name):
    params, rewards, special = _case(kind, name)
    syn = K.graph(K.SMALL, special=special)
    _, ob = K.pair(K.SMALL, syn, gpu=False, **params)
    emu = _emu_from(ob, K.SMALL[2])
    for k in ("w_prune", "p_new", "w_init", "compact_every"):
        emu.p[k] = getattr(ob.p, k)
    emu.capacity = int(ob.s.dims.syn_capacity)
    emu.stim = (0, 256)
    with np.errstate(all="ignore"):  # inf - inf, 0 * inf: the operations under test
        for k in range(10):
            if k in rewards:
                ob.set_reward(rewards[k])
                emu.reward = F(rewards[k])
            ob.pass_serial()
            emu.one_pass()
            _same_as_emu(ob, emu, f"{name} pass {k}")
    if name == "clock_inc=2,renorm_thresh=9":
        assert ob.renormalisations() >= 1
    if name == "plasticity":
        assert ob.stats()["pruned"] == emu.pruned > 0 and ob.stats()["grown"] == emu.n_grown > 0


@functools.lru_cache(maxsize=None)
def _wide(kind, name):
    """The serial oracle over the wide shape's GPU test, and what the
    conditions below need of every pass."""
    params, rewards, special = _case(kind, name)
    syn = K.graph(K.WIDE, special=special)
    log = []

    def each(k, o):
        log.append(dict(clock=o.clock, stats=o.stats(), renorms=o.renormalisations()))

    o = K.run_oracle(K.WIDE, syn, rewards, each=each, **params)
    return o, log


@pytest.mark.parametrize("kind,name", ALL_CASES, ids=IDS)
def test_threaded_equals_serial(kind, name):
    params, rewards, special = _case(kind, name)
    a, _ = _wide(kind, name)
    syn = K.graph(K.WIDE, special=special)
    _, b = K.pair(K.WIDE, syn, gpu=False, **params)
    for k in range(K.PASSES):
        K.set_rewards(k, rewards, b)
        b.pass_threaded(nthreads=5)
    K.same(b, a, name)
    assert a.stats() == b.stats()


NO_RECORD_MOVES = [c for c in ALL_CASES if not _case(*c)[0].get("compact_every")]


@pytest.mark.parametrize("kind,name", NO_RECORD_MOVES, ids=[f"{a}:{b}" for a, b in NO_RECORD_MOVES])
def test_two_shard_phases_equal_serial(kind, name):
    """test_oracle.test_shard_phases_equal_serial_full_sweep's harness: every
    shard sweeps its whole range, so the global order is the unsharded sweep's.
    (Not with structural plasticity: its update moves records within a shard
    only, so the shards' records are not the unsharded array's.)"""
    params, rewards, special = _case(kind, name)
    a, _ = _wide(kind, name)
    shards = [o for _, o in K.shard_pairs(K.WIDE, K.graph(K.WIDE, special=special), gpu=False, **params)]
    for k in range(K.PASSES):
        K.set_rewards(k, rewards, *shards)
        oracle_shard_pass(shards)
    got = np.concatenate([s.syn for s in shards])
    assert np.array_equal(got.view(np.uint32), a.syn.view(np.uint32)), name
    for s in shards:
        assert np.array_equal(s.last_fired, a.last_fired), name
        assert s.scalars()["clock"] == a.scalars()["clock"], name
        assert K.f32_bits(s.s.rbar) == K.f32_bits(a.s.rbar), name


# ---- c. the conditions of the GPU tests, on the oracle at their shapes --------------------------
def _busy(name, st):
    if name in K.GATES_EVERYTHING:
        assert st["post_gated"] == 0 and st["pre_gated"] > 0, (name, st)
        assert st["fired"] == 0 and st["updated"] == 0, (name, st)
    else:
        assert st["fired"] > 0 and st["updated"] > 0, (name, st)


@pytest.mark.parametrize("name", list(K.KNOBS))
def test_every_knob_case_stays_busy(name):
    o, log = _wide("knob", name)
    _busy(name, o.stats())
    clocks = [e["clock"] for e in log]
    if name == "clock_inc=2^31+1":
        assert max(clocks) > 2**32, clocks  # the u64 clock passes 2^32 at a compared pass
    if name == "clock_inc=2,renorm_thresh=9":
        assert log[-1]["renorms"] >= 2, [e["renorms"] for e in log]
    if name == "clock_inc=0":
        assert set(clocks) == {0}


@functools.lru_cache(maxsize=None)
def _large(name, passes=K.PASSES):
    params, rewards = K.KNOBS[name]
    return K.run_oracle(K.LARGE, K.graph(K.LARGE), rewards, passes=passes, **params).stats()


@pytest.mark.parametrize("name", K.LARGE_SHAPE)
def test_large_shape_knob_cases_stay_busy(name):
    _busy(name, _large(name))


@pytest.mark.parametrize("shape", ["WIDE", "LARGE"])
def test_window_7_8_9_differ_in_pre_gated(shape):
    """A fallback to k_bitmap that kept window_pre = 7's bitmap at 8 or 9 would show."""
    if shape == "WIDE":
        got = [_wide("knob", f"window_pre={w}")[0].stats()["pre_gated"] for w in (7, 8, 9)]
    else:
        got = [_large(f"window_pre={w}")["pre_gated"] for w in (7, 8, 9)]
    assert got[0] < got[1] < got[2], got


@pytest.mark.parametrize("name", ["random:" + k for k in K.CLOCK_AND_WINDOW])
def test_random_mode_knob_cases_stay_busy(name):
    name = name.split(":", 1)[1]
    params, rewards = K.KNOBS[name]
    o = K.run_oracle(K.RANDOM, K.graph(K.RANDOM, seed=5), rewards, mode=1, seed=9, **params)
    _busy(name, o.stats())


@pytest.mark.parametrize("name", list(K.RAW_KNOBS))
def test_raw_knob_cases_stay_busy(name):
    o = K.run_oracle(K.RAW, K.graph(K.RAW, seed=1), {2: 0.5}, passes=8, renorm_thresh=2**64 - 1, **K.RAW_KNOBS[name])
    _busy(name, o.stats())


def _stale_hidden(o, inc, window):
    """Hidden neurons that a spike list of the last `window` passes names and
    that are no longer recent: stamped, and window < age <= inc * window."""
    age = np.uint32(o.clock & 0xFFFFFFFF) - o.last_fired[512:].astype(np.uint32)
    return int(((o.last_fired[512:] > 0) & (age > window) & (age <= inc * window)).sum())


@pytest.mark.parametrize("shape", ["WIDE", "LARGE"])
@pytest.mark.parametrize("name", ["clock_inc=2", "clock_inc=3,window_pre=7", "clock_inc=2,renorm_thresh=9"])
def test_huge_budget_makes_the_clock_step_matter(shape, name):
    """What build_next_ok's clock_inc term protects: with a clock step above 1
    the spike lists of the last window_pre passes name neurons that have aged
    out.  Under the default budget there is none in any pass (the outputs of
    the dense block fire again first), under the huge one hundreds."""
    params, rewards = K.KNOBS[name]
    inc, window = params["clock_inc"], params.get("window_pre", 5)
    for budget, expect in (({}, False), (dict(max_spikes=K.HUGE_BUDGET), True)):
        stale = []
        K.run_oracle(getattr(K, shape), K.graph(getattr(K, shape)), rewards, **params, **budget,
                     each=lambda k, o: stale.append(_stale_hidden(o, inc, window)))
        assert (max(stale) >= 100) == expect and (expect or max(stale) == 0), (budget, stale)


@pytest.mark.parametrize("shape", ["WIDE", "LARGE"])
def test_huge_budget_window_7_8_9_differ_through_hidden_neurons(shape):
    """... and the window_pre edges differ in the records that hidden neurons
    pre-gate (src >= 512), which the default budget never makes recent again
    once the creation zeros have aged out."""
    shape = getattr(K, shape)
    syn = K.graph(shape)
    hidden_src = syn["src"] >= 512
    got = []
    for w in (7, 8, 9):
        late = []

        def each(k, o, w=w, late=late):
            if o.clock > w + 1:  # the creation zeros are no longer recent at the next pass
                age = np.uint32(o.clock) - o.last_fired.astype(np.uint32)
                late.append(int(((age <= w)[syn["src"]] & hidden_src).sum()))

        o = K.run_oracle(shape, syn, K.REWARDS, window_pre=w, max_spikes=K.HUGE_BUDGET, each=each)
        _busy(f"window_pre={w}", o.stats())
        got.append(sum(late))
    assert min(got) > 0 and len(set(got)) == 3, got


@pytest.mark.parametrize("window", [7, 1])
@pytest.mark.parametrize("hold", [1, 2])
def test_rotating_stimulus_stays_busy(window, hold):
    _, o = K.pair(K.LARGE, K.graph(K.LARGE), gpu=False, window_pre=window, max_spikes=K.HUGE_BUDGET)
    for k in range(20):
        K.set_rewards(k, K.REWARDS, o)
        o.set_auto_stimulus(*K.rotating_stimulus(k // hold))
        o.pass_threaded(nthreads=16)
    _busy("rotating", o.stats())


def test_rotating_stimulus_fills_the_stimulus_ring():
    """Passes p-6 .. p+1 hold 8 distinct ranges (window_pre = 7 reads them all)."""
    ranges = [K.rotating_stimulus(k) for k in range(20)]
    assert any(len(set(ranges[p - 6:p + 2])) == 8 for p in range(6, 19))
    assert all(0 <= f and f + c <= 512 for f, c in ranges)  # inputs, and outputs for the later ones


def _changed_classes(shape, params, passes, mode=0, graph_seed=7):
    """Per class, the records whose weight one pass changed, summed over the
    passes that move no record (the class is that of the weight before the
    pass), "+0 to -0" among them; the final records; which were ever changed;
    the statistics."""
    syn = K.graph(shape, seed=graph_seed, special=True)
    _, o = K.pair(shape, syn, gpu=False, **(K.random_mode(params) if mode else params))
    total = dict.fromkeys(K.weight_classes(syn["w"]), 0)
    total["+0 to -0"] = 0
    changed_ever = np.zeros(len(syn), bool)
    for k in range(passes):
        K.set_rewards(k, K.REWARDS, o)
        before = o.syn.copy()
        K.oracle_step(o, shape)
        ce = params.get("compact_every", 0)
        if ce and (k + 1) % ce == 0:
            continue  # a structural update moved records
        changed = before["w"].view(np.uint32) != o.syn["w"].view(np.uint32)
        if not ce:
            changed_ever |= changed
        for c, m in K.weight_classes(before["w"]).items():
            total[c] += int((m & changed).sum())
        total["+0 to -0"] += int(((before["w"].view(np.uint32) == 0) & (o.syn["w"].view(np.uint32) == 0x80000000)).sum())
    return total, o.syn.copy(), changed_ever, o.stats()


# (structural plasticity runs at tests/test_gpu_plasticity.py's shapes: WIDE, and RANDOM_SP for RANDOM)
WEIGHT_RUNS = [(s, n) for n in K.WEIGHT_CASES for s in (("WIDE", "RANDOM") if n == "plasticity" else ("LARGE", "WIDE", "RANDOM"))]
WEIGHT_RUNS.append(("RAW", "default"))  # the buffer-index launcher's


@pytest.mark.parametrize("shape,name", WEIGHT_RUNS)
def test_every_special_class_reaches_the_update(shape, name):
    params = K.WEIGHT_CASES[name]
    if shape == "RANDOM":
        total, syn, ever, st = _changed_classes(K.random_shape(params), params, K.PASSES, mode=1, graph_seed=5)
    else:
        total, syn, ever, st = _changed_classes(getattr(K, shape), params, 8, graph_seed=1 if shape == "RAW" else 7)
    assert all(n > 0 for c, n in total.items() if c != "+0 to -0"), total
    assert st["fired"] > 0 and st["updated"] > 0, st
    if name == "plasticity":
        assert st["pruned"] > 0 and st["grown"] > 0, st
    w = syn["w"]
    if name == "w_max=inf":
        cls = K.weight_classes(w[ever])
        assert cls["subnormal"].any(), "no updated weight is subnormal afterwards"
    if name == "w_min=-0":  # clampf's select gives lo = -0 for x = +0, where a max instruction may keep +0
        assert total["+0 to -0"] > 0, "no weight that was +0 before a pass is -0 after it"
    if name == "w=+-3e38":
        with np.errstate(invalid="ignore"):
            assert ((w[ever] < -1) | (w[ever] > 2)).any(), "no updated weight outside [-1, 2]"
