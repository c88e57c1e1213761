"""Test helpers for parity off the default knobs (plain numpy, no GPU).

Almost every parity test runs the reference's default abnn_params on generator
weights (in [0.1, 0.2] and [0.4, 0.8], which the clamp then keeps in
[0.001, 1]).  The library accepts any clock_inc, window_pre, refractory and
float knob, and a loaded file may hold any weight bits.  This module holds

* `KNOBS`: the knob cases (what is not named stays at the default), each with
  its reward schedule {pass: reward, set before that pass},
* `WEIGHT_CASES`: the knobs under which the special weights are traversed,
* `special_weights`: every third record's weight replaced by NaNs, infinities,
  zeros, subnormals, negative and large values,
* `pair` / `same`: a GPU handle and an OracleBrain built alike, and their
  comparison on bits (a NaN's payload and a zero's sign count),
* the two shapes the GPU tests use and the pass loops shared by them and by
  the oracle-only tests of their conditions (tests/test_knob_model.py).
"""
from __future__ import annotations

import functools

import numpy as np

U32_MAX = 2**32 - 1
REWARDS = {4: 0.5, 8: -3.0}
INF, NAN = float("inf"), float("nan")

# id -> (knobs, reward schedule)
KNOBS = {
    "clock_inc=0": (dict(clock_inc=0), REWARDS),
    "clock_inc=2": (dict(clock_inc=2), REWARDS),
    "clock_inc=3,window_pre=7": (dict(clock_inc=3, window_pre=7), REWARDS),
    "clock_inc=2^31+1": (dict(clock_inc=2**31 + 1, renorm_thresh=2**64 - 1), REWARDS),
    "clock_inc=2,renorm_thresh=9": (dict(clock_inc=2, renorm_thresh=9), REWARDS),
    "window_pre=1": (dict(window_pre=1), REWARDS),
    "window_pre=7": (dict(window_pre=7), REWARDS),
    "window_pre=8": (dict(window_pre=8), REWARDS),
    "window_pre=9": (dict(window_pre=9), REWARDS),
    "window_pre=40": (dict(window_pre=40), REWARDS),
    "window_pre=2^32-1": (dict(window_pre=U32_MAX), REWARDS),
    "refractory=2^32-1": (dict(refractory=U32_MAX), REWARDS),
    "refractory=7,window_pre=7": (dict(refractory=7, window_pre=7), REWARDS),
    "w_max=2": (dict(w_min=0.0, w_max=2.0, a_ltp=0.5), REWARDS),
    "w_crossed": (dict(w_min=0.3, w_max=0.2), REWARDS),
    "w_min=-1": (dict(w_min=-1.0, a_ltd=1.5), REWARDS),
    "reward_knobs": (dict(eta_reward=0.5, alpha_rbar=0.5, target_rate_hz=0.0, eta_home=1e-3), REWARDS),
    "reward=inf": ({}, {4: INF}),
    "reward=nan": ({}, {4: NAN}),
    "reward=+-3e38": (dict(eta_reward=10.0), {4: 3e38, 6: -3e38}),
}
GATES_EVERYTHING = ("clock_inc=0", "refractory=2^32-1")  # nothing leaves the refractory gate
CLOCK_AND_WINDOW = tuple(k for k in KNOBS if k.startswith(("clock_inc", "window_pre")))
# the cases that need many gate ranges, long candidate lists and the look-back
LARGE_SHAPE = ("clock_inc=3,window_pre=7", "window_pre=1", "window_pre=7", "window_pre=8", "window_pre=9",
               "window_pre=2^32-1")

# the buffer-index launcher's cases (its host decides renormalisation; reward 0.5 from pass 2)
RAW_KNOBS = {
    "clock_inc=3": dict(clock_inc=3),
    "window_pre=1": dict(window_pre=1),
    "window_pre=7": dict(window_pre=7),
    "window_pre=40": dict(window_pre=40),
    "refractory=2^32-1": dict(refractory=U32_MAX),
    "w_crossed": dict(w_min=0.3, w_max=0.2),
    "w_max=2": dict(w_min=0.0, w_max=2.0),
}

SP = dict(w_prune=0.105, p_new=0.35, w_init=0.5, compact_every=2, seed=13)  # tests/test_gpu_plasticity.py
WEIGHT_CASES = {
    "default": {},
    "w_max=inf": dict(w_min=0.0, w_max=INF),
    "w=+-3e38": dict(w_min=-3e38, w_max=3e38),
    "base_scale=3": dict(base_scale=3.0),
    # x = +0 against lo = -0: the select `x > lo ? x : lo` gives -0 where a max instruction may keep +0
    "w_min=-0": dict(w_min=-0.0),
    "plasticity": SP,
}

# {n_hidden, records, events}: the suite's two parity shapes, config 1 (the
# Python restatement's) and test_random_collisions_every_pass's
WIDE = (3000, 120_000, 120_000)
LARGE = (99_488, 1_000_000, 1_000_000)
SMALL = (488, 10_000, 100_000)
RANDOM = (488, 2_000, 12_000)
RANDOM_SP = (3000, 120_000, 60_000)  # random mode with structural plasticity (tests/test_gpu_plasticity.py)
RAW = (9_488, 200_000, 150_000)  # the buffer-index launcher's (tests/test_gpu_raw.py)
PASSES = 12
HUGE_BUDGET = 200_000  # a max_spikes no sweep here exhausts: spikes far into the array, every pass


# ---- the special weights -----------------------------------------------------------------------
def _f32(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


SPECIAL_BITS = np.array([
    0x7FC00000,  # a quiet NaN
    0xFFC00001,  # a NaN with a sign and a payload
    0x7F800000, 0xFF800000,  # +inf, -inf
    0x00000000, 0x80000000,  # +0, -0
    np.float32(1e-40).view(np.uint32), np.float32(-1e-40).view(np.uint32),  # subnormals
    0x00000001,  # 1.4e-45, the least subnormal
    np.float32(-0.5).view(np.uint32), np.float32(1.5).view(np.uint32), np.float32(3e38).view(np.uint32),
    np.float32(1e-20).view(np.uint32), np.float32(0.7).view(np.uint32),
], dtype=np.uint32)
assert _f32(1) == np.float32(1.4e-45) and np.isnan(_f32(0xFFC00001))


def special_weights(syn):
    """`syn` with the weight of every third record (i % 3 == 0) replaced, in
    turn, by SPECIAL_BITS; written as bits, returns the array."""
    at = np.arange(0, len(syn), 3)
    w = syn["w"].view(np.uint32)
    w[at] = SPECIAL_BITS[np.arange(at.size) % SPECIAL_BITS.size]
    return syn


def weight_classes(w):
    """The special classes of fp32 weights, as {name: mask}."""
    w = np.asarray(w, dtype=np.float32)
    a = np.abs(w)
    with np.errstate(invalid="ignore"):
        return {
            "nan": np.isnan(w),
            "inf": np.isinf(w),
            "subnormal": (a > 0) & (a < np.finfo(np.float32).tiny),
            "zero": w == 0,
            "negative": np.isfinite(w) & (w < 0),
            "above_1": np.isfinite(w) & (w > 1),
        }


# ---- graphs ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def _graph(n_nrn, n_syn, seed, special):
    from oracle import oracle as O

    syn = O.gen_synapses(0, n_syn, 256, 256, n_nrn, seed, nthreads=16)
    if special:
        special_weights(syn)
    syn.setflags(write=False)
    return syn


def graph(shape, seed=7, special=False):
    """The generated graph of a shape (a fresh copy), with the special weights or not."""
    return _graph(512 + shape[0], shape[1], seed, bool(special)).copy()


# ---- a GPU handle and an oracle built alike ----------------------------------------------------
def pair(shape, syn, gpu=True, syn_offset=0, global_events=0, **params):
    """(abnn_amd.Brain or None, OracleBrain) over 256 + 256 + shape[0] neurons
    holding `syn`, the stimulus on all inputs.  With structural plasticity
    the capacity is 20 000 records above the size (tests/test_gpu_plasticity.py)."""
    from oracle import oracle as O

    n_hidden, _, events = shape
    syn_capacity = len(syn) + 20_000 if params.get("compact_every") else 0
    g = None
    if gpu:
        import abnn_amd

        g = abnn_amd.Brain(256, 256, n_hidden, len(syn), events, syn_offset=syn_offset, global_events=global_events,
                           syn_capacity=syn_capacity, **params)
        g.upload_synapses(syn)
        g.set_auto_stimulus(0, 256)
    o = O.OracleBrain(256, 256, n_hidden, len(syn), events, syn_offset=syn_offset, global_events=global_events,
                      syn_capacity=syn_capacity, **params)
    o.set_synapses(syn)
    o.set_auto_stimulus(0, 256)
    return g, o


def shard_pairs(shape, syn, world=2, gpu=True, **params):
    """`world` shards of `syn`, every shard sweeping its whole range: [(g, o)]."""
    from abnn_amd.shard import global_events, shard_ranges

    ge = global_events(len(syn), shape[2], world, params.get("mode", 0))
    return [pair(shape, syn[lo:hi], gpu=gpu, syn_offset=lo, global_events=ge, **params)
            for lo, hi in shard_ranges(len(syn), world)]


def random_mode(params):
    """The knobs of a case in random mode (seed 9 unless the case names one)."""
    return dict(params, mode=1, seed=params.get("seed", 9))


def random_shape(params):
    return RANDOM_SP if params.get("compact_every") else RANDOM


def f32_bits(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def same(g, o, what=""):
    """g (a handle, or another oracle) equals o on bits: record count, records
    as u32 words, lastFired as u64, clock, pass_index, rBar's bits."""
    oracle = not hasattr(g, "download_synapses")
    n_g = int(g.s.dims.n_syn) if oracle else g.n_syn()
    assert n_g == int(o.s.dims.n_syn), f"n_syn {what}"
    got = g.syn if oracle else g.download_synapses()
    differ = np.flatnonzero((got.view(np.uint32).reshape(-1, 4) != o.syn.view(np.uint32).reshape(-1, 4)).any(axis=1))
    assert differ.size == 0, (f"synapses differ {what}: {differ.size} records, the first at {differ[0]}: "
                              f"{got[differ[0]]} ({got['w'].view(np.uint32)[differ[0]]:#x}) != "
                              f"{o.syn[differ[0]]} ({o.syn['w'].view(np.uint32)[differ[0]]:#x})")
    lf = g.last_fired if oracle else g.last_fired()
    assert np.array_equal(lf, o.last_fired), f"lastFired differs {what}"
    sg, so = g.scalars(), o.scalars()
    assert (sg["clock"], sg["pass_index"]) == (so["clock"], so["pass_index"]), f"{what}: {sg} != {so}"
    assert f32_bits(sg["rbar"]) == f32_bits(so["rbar"]), f"rbar {what}: {f32_bits(sg['rbar']):#x} != {f32_bits(so['rbar']):#x}"
    return lf


def set_rewards(k, rewards, *brains):
    """The schedule's reward of pass k, if any, on every brain."""
    if k in rewards:
        for b in brains:
            b.set_reward(rewards[k])


def oracle_step(o, shape):
    """One oracle pass: serial at the small shapes, 16 threads at the large one."""
    if shape == LARGE:
        o.pass_threaded(nthreads=16)
    else:
        o.pass_serial()


def run_oracle(shape, syn, rewards, passes=PASSES, each=None, **params):
    """The oracle alone over a GPU test's passes; each(k, o) after every pass."""
    _, o = pair(shape, syn, gpu=False, **params)
    for k in range(passes):
        set_rewards(k, rewards, o)
        oracle_step(o, shape)
        if each:
            each(k, o)
    return o


def rotating_stimulus(k):
    """The auto-stimulus range before pass k of the rotating-stimulus tests."""
    return (k * 32) % 256, 200
