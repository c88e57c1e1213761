"""The pinned slice of the sweep's record stream (engine.h pin_k,
ABNN_STREAM_PIN_MB): iterations whose index mod 16 is below pin_k are read with
ordinary loads, the others non-temporally.  The slice is a load policy and
nothing more, so every result stays what the CPU oracle computes, on bits:
records, lastFired, scalars, statistics -- with no slice, a part of the stream
and all of it, over a partial last iteration and empty ranges, and across
structural updates that move records inside pinned lines.  On a graph of 2^21
records with config 2's neuron counts; the oracle's runs are shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import knob_helpers as K

pytestmark = pytest.mark.gpu

N_SYN = 1 << 21
N_HIDDEN = 99_488
FULL = (N_HIDDEN, N_SYN, N_SYN)  # 4096 iterations of 512 events: 3 B x 2^21 = 6 MiB of stream
ODD = (N_HIDDEN, N_SYN, 1_000_192)  # 1953.5 iterations: a partial last one, ranges of one iteration and of none
SP = dict(w_prune=0.105, p_new=0.35, w_init=0.5, compact_every=4, seed=13)  # tests/test_gpu_plasticity.py's, every 4 passes


def pin_k(g):
    f = g._lib.abnn_debug_stream_pin
    f.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    f.restype = C.c_int
    k = C.c_uint32(99)
    assert f(g._h, C.byref(k)) == 0
    return k.value


def expected_pin_k(mib, events):
    return min(16, 16 * (mib << 20) // (3 * events))


@functools.lru_cache(maxsize=None)
def oracle_run(shape, passes, params):
    """The oracle over `passes` passes: per pass {lastFired, scalars, record
    count}, and at the end the records and the statistics."""
    _, o = K.pair(shape, K.graph(shape), gpu=False, **dict(params))
    per_pass = []
    for k in range(passes):
        K.set_rewards(k, K.REWARDS, o)
        o.pass_threaded(nthreads=16)
        per_pass.append((o.last_fired.copy(), o.scalars(), int(o.s.dims.n_syn)))
    return per_pass, o.syn[:int(o.s.dims.n_syn)].copy(), o.stats()


def run_against_oracle(monkeypatch, mib, shape, passes, want_k, **params):
    monkeypatch.setenv("ABNN_STREAM_PIN_MB", str(mib))
    per_pass, syn, stats = oracle_run(shape, passes, tuple(sorted(params.items())))
    g, _ = K.pair(shape, K.graph(shape), **params)
    assert pin_k(g) == want_k
    for k in range(passes):
        K.set_rewards(k, K.REWARDS, g)
        g.encode_traversal(1)
        lf, sc, n = per_pass[k]
        assert g.n_syn() == n, f"n_syn, pass {k}"
        assert np.array_equal(g.last_fired(), lf), f"lastFired, pass {k}"
        sg = g.scalars()
        assert (sg["clock"], sg["pass_index"]) == (sc["clock"], sc["pass_index"]), f"pass {k}: {sg} != {sc}"
        assert K.f32_bits(sg["rbar"]) == K.f32_bits(sc["rbar"]), f"rbar, pass {k}"
    got = g.download_synapses()
    assert np.array_equal(got.view(np.uint32), syn.view(np.uint32)), "records"
    assert g.stats() == stats
    return g


@pytest.mark.parametrize("mib,want_k", [(0, 0), (2, 5), (6, 16)])
def test_slice_of_none_part_and_all(gpu, monkeypatch, mib, want_k):
    assert expected_pin_k(mib, FULL[2]) == want_k
    run_against_oracle(monkeypatch, mib, FULL, 8, want_k)


def test_partial_last_iteration_and_empty_ranges(gpu, monkeypatch):
    """1,000,192 events are 1953 iterations and 256 events; the ranges (one per
    wave) outnumber them, so some are empty and the others hold one: the
    prefetch two iterations ahead reads the dummy block at a pinned index."""
    assert ODD[2] % 512 == 256 and expected_pin_k(1, ODD[2]) == 5
    g = run_against_oracle(monkeypatch, 1, ODD, 8, 5)
    assert g.visited_events() == ODD[2]


def test_records_move_inside_pinned_lines(gpu, monkeypatch):
    """Pruning, synaptogenesis and a structural update every 4 passes: the
    update moves records inside lines the last pass left in the cache, and the
    next pass must read the moved ones."""
    g = run_against_oracle(monkeypatch, 2, FULL, 12, 5, **SP)
    st = g.stats()
    assert st["pruned"] > 0 and st["grown"] > 0 and g.structural_updates() >= 2
    assert pin_k(g) == expected_pin_k(2, g.visited_events())  # recomputed with the sweep's length


@pytest.mark.parametrize("params", [dict(track_visits=1), dict(mode=1, seed=9)], ids=["track_visits", "random"])
def test_no_slice_with_track_visits_or_random_mode(gpu, monkeypatch, params):
    monkeypatch.setenv("ABNN_STREAM_PIN_MB", "4096")
    shape = K.WIDE
    g, o = K.pair(shape, K.graph(shape), **params)
    assert pin_k(g) == 0
    for k in range(3):
        g.encode_traversal(1)
        o.pass_serial()
        K.same(g, o, f"{params} pass {k}")
    assert g.stats() == o.stats()
    assert pin_k(g) == 0
