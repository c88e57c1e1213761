"""GPU parity off the default knobs (tests/knob_helpers.py): clock_inc other
than 1, the edges of window_pre, refractory and the float knobs at values no
other test tries, non-finite rewards, and weights that are NaN, infinite,
zero, subnormal, negative or above 1 -- HIP path against the CPU oracle after
every pass, on bits (records as u32 words, lastFired, clock, pass_index,
rBar's bits), the statistics at the end.  tests/test_knob_model.py asserts on
the oracle alone that every case here stays busy and that every class of
special weight reaches the update."""
import numpy as np
import pytest

import high_id_helpers as H
import knob_helpers as K
from shard_helpers import GpuShards, oracle_shard_pass

pytestmark = pytest.mark.gpu

ENVS = {"two-kernel": {"ABNN_FUSED": "0"}, "spec-everywhere": {"ABNN_SPEC": "2"}}


def _shape_of(name):
    return K.LARGE if name in K.LARGE_SHAPE else K.WIDE


def _every_pass(g, o, shape, rewards, window, passes=K.PASSES, what="", stim=None, before=None):
    """Every pass: the state against the oracle's, and the pass's exact recent
    bitmap against the one recomputed from the pass-start lastFired.  Returns
    which passes built the next pass's bitmap from the spike lists."""
    lf, modes = g.last_fired(), []
    for k in range(passes):
        K.set_rewards(k, rewards, g, o)
        first, count = stim(k) if stim else (0, 256)
        if stim:
            g.set_auto_stimulus(first, count)
            o.set_auto_stimulus(first, count)
        now = g.scalars()["clock"]
        if before:
            before(k, now, lf)
        lf[first:first + count] = now  # the stimulus is stamped at pass start
        g.encode_traversal(1)
        K.oracle_step(o, shape)
        bm, inc_next = H._bitmap(g)
        modes.append(inc_next)
        assert np.array_equal(bm, H._expected_bitmap(lf, now, bm.size, window)), f"bitmap, {what} pass {k}"
        lf = K.same(g, o, f"{what} pass {k}")
    assert g.stats() == o.stats(), what
    return modes


# With the default budget the dense input -> output block at the head of the
# array takes every spike, and its outputs fire again before they age out: no
# neuron is ever in a spike list of the window and no longer recent.  With a
# budget the sweep never exhausts, hidden neurons fire now and then for the
# whole run (tests/test_knob_model.py asserts it), so a bitmap built from the
# wrong lists, or for the wrong clock step, differs from the exact one.
BUDGETS = {"budget-default": {}, "budget-huge": dict(max_spikes=K.HUGE_BUDGET)}


def _knob_case(name, shape, monkeypatch, env, budget="budget-default"):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    params, rewards = K.KNOBS[name]
    g, o = K.pair(shape, K.graph(shape), **params, **BUDGETS[budget])
    return _every_pass(g, o, shape, rewards, params.get("window_pre", H.WINDOW_PRE), what=f"{name} {env} {budget}")


# ---- the knob cases ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.KNOBS))
def test_knobs_fused(gpu, monkeypatch, name):
    """Every case on the default fused pass, at the wide shape."""
    modes = _knob_case(name, K.WIDE, monkeypatch, {})
    params = K.KNOBS[name][0]
    window = params.get("window_pre", H.WINDOW_PRE)
    if params.get("clock_inc", 1) != 1 or window >= 8:
        assert not any(modes), modes  # capi.hip build_next_ok: every bitmap by k_bitmap
    else:
        assert modes[-1], modes  # ... and here, in the end, by the spike lists


@pytest.mark.parametrize("budget", list(BUDGETS))
@pytest.mark.parametrize("name", K.LARGE_SHAPE)
def test_knobs_fused_large(gpu, monkeypatch, name, budget):
    """The window_pre edges and clock_inc = 3 over many gate ranges."""
    _knob_case(name, K.LARGE, monkeypatch, {}, budget)


@pytest.mark.parametrize("name", [n for n in K.CLOCK_AND_WINDOW if n not in K.LARGE_SHAPE])
def test_clock_and_window_fused_huge_budget(gpu, monkeypatch, name):
    _knob_case(name, K.WIDE, monkeypatch, {}, "budget-huge")


@pytest.mark.parametrize("budget", list(BUDGETS))
@pytest.mark.parametrize("env", list(ENVS))
@pytest.mark.parametrize("name", K.CLOCK_AND_WINDOW)
def test_clock_and_window_other_passes(gpu, monkeypatch, name, env, budget):
    """The two-kernel pass, and speculative stores everywhere."""
    _knob_case(name, _shape_of(name), monkeypatch, ENVS[env], budget)


def _shards_every_pass(shape, syn, rewards, what, **params):
    import torch

    pairs = K.shard_pairs(shape, syn, **params)
    gs, obs = GpuShards([g for g, _ in pairs]), [o for _, o in pairs]
    for k in range(K.PASSES):
        K.set_rewards(k, rewards, *gs.brains, *obs)
        gs.pass_()
        oracle_shard_pass(obs)
        torch.cuda.synchronize()
        for r, (g, o) in enumerate(pairs):
            K.same(g, o, f"{what} shard {r} pass {k}")
    for g, o in pairs:
        assert g.stats() == o.stats(), what
    return obs


@pytest.mark.parametrize("budget", list(BUDGETS))
@pytest.mark.parametrize("name", K.CLOCK_AND_WINDOW)
def test_clock_and_window_two_virtual_shards(gpu, name, budget):
    params, rewards = K.KNOBS[name]
    shape = _shape_of(name)
    _shards_every_pass(shape, K.graph(shape), rewards, f"{name} {budget}", **params, **BUDGETS[budget])


def _random_every_pass(shape, syn, rewards, what, **params):
    g, o = K.pair(shape, syn, **K.random_mode(params))
    for k in range(K.PASSES):
        K.set_rewards(k, rewards, g, o)
        g.encode_traversal(1)
        o.pass_serial()
        K.same(g, o, f"{what} pass {k}")
    assert g.stats() == o.stats(), what
    assert g.visited_events() == shape[2]
    return g, o


@pytest.mark.parametrize("name", K.CLOCK_AND_WINDOW)
def test_clock_and_window_random_mode(gpu, name):
    """~6 picks per record and pass: colliding stores every pass."""
    params, rewards = K.KNOBS[name]
    _random_every_pass(K.RANDOM, K.graph(K.RANDOM, seed=5), rewards, name, **params)


# ---- the rotating stimulus -----------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, ENVS["two-kernel"]], ids=["fused", "two-kernel"])
@pytest.mark.parametrize("variant", ["every-pass", "every-pass+host-write", "every-2nd-pass"])
@pytest.mark.parametrize("window", [7, 1])
def test_rotating_stimulus(gpu, monkeypatch, window, variant, env):
    """Another auto-stimulus range before every pass: the incremental build
    reads the distinct ranges of the last window_pre passes and this one's
    (capi.hip plan_build), and the next pass, whose range is new, must not
    take the bitmap built for the old one.  With the range held for two
    passes, every second pass does take it, built from several ranges.  With a
    set_last_fired at pass 10, the build drops back to k_bitmap and comes
    back (build_next_ok)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g, o = K.pair(K.LARGE, K.graph(K.LARGE), window_pre=window, max_spikes=K.HUGE_BUDGET)  # (BUDGETS above)
    host_write = variant.endswith("host-write")
    hold = 2 if variant == "every-2nd-pass" else 1

    def write(k, now, lf):
        if host_write and k == 10:
            v = np.full(1000, now - 1, np.uint64)
            v[::7] = now + 2  # not recent until the clock gets there
            g.set_last_fired(v, 5000)
            o.last_fired[5000:6000] = v
            lf[5000:6000] = v

    modes = _every_pass(g, o, K.LARGE, K.REWARDS, window, passes=20, what=f"W={window} {variant} {env}",
                        stim=lambda k: K.rotating_stimulus(k // hold), before=write)
    # (which builder: the bitmap itself is compared above, every pass)
    assert modes[9] and modes[-1], modes  # built from the spike lists before the write, and again at the end
    assert not host_write or not modes[10], modes  # the write dropped the build back to k_bitmap


# ---- the special weights -------------------------------------------------------------------------
def _weight_case(name, shape, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    params = K.WEIGHT_CASES[name]
    shape = K.WIDE if name == "plasticity" else shape  # tests/test_gpu_plasticity.py's shape
    g, o = K.pair(shape, K.graph(shape, special=True), **params)
    _every_pass(g, o, shape, K.REWARDS, H.WINDOW_PRE, what=f"weights {name} {env}")
    return g, o


@pytest.mark.parametrize("env", [{}, *ENVS.values()], ids=["fused", *ENVS])
@pytest.mark.parametrize("name", list(K.WEIGHT_CASES))
def test_special_weights(gpu, monkeypatch, name, env):
    g, o = _weight_case(name, K.LARGE, monkeypatch, env)
    if name == "plasticity":
        st = o.stats()
        assert st["pruned"] > 0 and st["grown"] > 0 and g.structural_updates() >= 2


@pytest.mark.parametrize("name", list(K.WEIGHT_CASES))
def test_special_weights_two_virtual_shards(gpu, name):
    shape = K.WIDE if name == "plasticity" else K.LARGE
    _shards_every_pass(shape, K.graph(shape, special=True), K.REWARDS, name, **K.WEIGHT_CASES[name])


@pytest.mark.parametrize("name", list(K.WEIGHT_CASES))
def test_special_weights_random_mode(gpu, name):
    """Colliding stores of NaN and subnormal weights (k_claim: the highest
    event wins); with structural plasticity, at the shape of
    test_gpu_plasticity's random-mode case, also their pruning (a NaN is never
    below w_prune) and the structural update."""
    params = K.WEIGHT_CASES[name]
    shape = K.random_shape(params)
    g, o = _random_every_pass(shape, K.graph(shape, seed=5, special=True), K.REWARDS, name, **params)
    if name == "plasticity":
        st = o.stats()
        assert st["pruned"] > 0 and st["grown"] > 0 and g.structural_updates() >= 2


def test_census_degrees_select_of_traversed_special_weights(gpu, monkeypatch):
    """After the last pass the records hold what the traversal made of the
    special weights next to the ones it never updated: the three device-side
    queries against their numpy references on the download."""
    from abnn_amd import census, degree, select

    g, _ = _weight_case("w=+-3e38", K.LARGE, monkeypatch, {})
    syn = g.download_synapses()
    n_nrn = g.n_neuron()
    cls = K.weight_classes(syn["w"])
    assert all(m.any() for m in cls.values()), {c: int(m.sum()) for c, m in cls.items()}
    for kw in (dict(), dict(src=(0, 256)), dict(dst=(512, 50_000))):
        for lo, hi in ((0.0, 1.0), (-2.0, 2.0)):
            want = census.reference(syn, census.config(64, lo, hi, **kw))
            assert want["nan"] > 0 and want["under"] > 0 and want["over"] > 0, kw
            got = g.census(64, lo, hi, **kw)
            assert np.array_equal(census.to_words(got), census.to_words(want)), (kw, lo, hi)
    what = ("out", "out_w", "in", "in_w")
    for r in (None, (0, 512), (512, 3000), (40_000, 7000)):  # (7000: more than the LDS planes hold)
        want = degree.reference(syn, degree.config(r, what), n_nrn)
        assert want["out_skipped"] > 0 and want["in_skipped"] > 0, r
        got = g.degrees(r, what)
        assert np.array_equal(degree.to_words(got), degree.to_words(want)), r
    for kw in (dict(weights=(-1.0, 1e-30)), dict(weights=(1.0, float("inf"))), dict(weights=(0.0, 1e-38), src=(0, 256)),
               dict(weights=(-float("inf"), 0.0), dst=(512, 50_000), any=True)):
        cfg = select.config(**kw)
        matched = int(select.matches(syn, cfg).sum())
        assert matched > 0, kw
        want = select.reference(syn, cfg, matched, n_nrn)
        got = g.select(**kw)
        assert got["matched"] == matched and got["written"] == matched, kw
        assert np.array_equal(got["index"], want["index"]), kw
        assert np.array_equal(got["syn"].view(np.uint32), want["syn"].view(np.uint32)), kw
        assert np.array_equal(select.to_words(got), select.to_words(want)), kw


def test_special_weights_round_trip(gpu, tmp_path):
    """upload / download, save / load and save_flat / load_flat keep every bit."""
    import abnn_amd

    syn = K.graph(K.WIDE, special=True)
    want = syn.view(np.uint32)
    n_hidden, n, events = K.WIDE

    def fresh():
        return abnn_amd.Brain(256, 256, n_hidden, n, events)

    g = fresh()
    g.upload_synapses(syn)
    assert np.array_equal(g.download_synapses().view(np.uint32), want), "upload -> download"
    g.save_flat(tmp_path / "m.flat")
    h = fresh()
    h.load_flat(tmp_path / "m.flat")
    assert np.array_equal(h.download_synapses().view(np.uint32), want), "save_flat -> load_flat"
    g.save(tmp_path / "m.bnn")
    h2 = fresh()
    h2.load(tmp_path / "m.bnn")
    assert np.array_equal(h2.download_synapses().view(np.uint32), want), "save -> load"
