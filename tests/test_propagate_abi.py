"""CPU checks of signal propagation (abnn.h abnn_propagate_*): the config
checks, the library's host rule (abnn_propagate_host, abnn_propagate_rescale_host:
csrc/propagate.h, the code the kernels share) against the numpy restatement of
abnn_amd.propagate word for word, known answers, the merge of shard results and
the ctypes mirror's layout."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from propagate_helpers import F32, I32_MAX, I32_MIN, NONE
from propagate_helpers import plane as _x
from propagate_helpers import records as _records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def _configs(n_nrn):
    from abnn_amd import propagate as P

    third = n_nrn // 3
    return [P.config(), P.config(reverse=True), P.config(fire_p=True), P.config(reverse=True, fire_p=True),
            P.config(weights=(-0.5, 0.6)), P.config(weights=(-INF, INF), fire_p=True),
            P.config(inputs=(third, third)), P.config(outputs=(5, 1)), P.config(inputs=(0, third), outputs=(third, n_nrn - third)),
            P.config(inputs=(n_nrn - 7, 7), outputs=(0, third), reverse=True, weights=(0.0, 200.5)),
            P.config(inputs=(third, third), outputs=(third, third), fire_p=True)]


def test_words_against_n_words_and_the_invalid_cases():
    from abnn_amd import _lib
    from abnn_amd import propagate as P

    lib = _lib.load()
    n_nrn = 1000

    def both(cfg, n=n_nrn):
        got = int(lib.abnn_propagate_words(C.byref(cfg), n))
        assert got == P.n_words(cfg, n), (got, P.n_words(cfg, n))
        return got

    assert both(P.config()) == 8 + 1000
    assert both(P.config(outputs=(10, 17))) == 8 + 17
    assert both(P.config(inputs=(0, 1000), outputs=(999, 1), reverse=True, fire_p=True, weights=(-INF, INF))) == 9
    for cfg in _configs(n_nrn):
        assert both(cfg) > 8
    assert int(lib.abnn_propagate_words(None, n_nrn)) == 0
    bad = [P.config(inputs=(5, 0)), P.config(outputs=(5, 0)), P.config(inputs=(999, 2)), P.config(outputs=(0, 1001)),
           P.config(weights=(0.5, 0.5)), P.config(weights=(0.6, 0.5)), P.config(weights=(float("nan"), 1.0)),
           P.config(weights=(0.0, float("nan")))]
    c = P.config()
    c.flags = 8  # an unknown bit
    bad.append(c)
    c = P.config()
    c.w_hi = 1.0  # bounds without WEIGHT
    bad.append(c)
    c = P.config()
    c.w_lo = -0.0  # ... even a negative zero
    bad.append(c)
    for k in range(5):
        c = P.config()
        c.reserved[k] = 1
        bad.append(c)
    for cfg in bad:
        assert both(cfg) == 0
    assert both(P.config(), 0) == 0 and both(P.config(), 1 << 32) == 0
    # the host entry points refuse them too
    x = np.zeros(n_nrn, dtype=np.int32)
    out = np.zeros(8 + n_nrn, dtype=np.uint64)
    for cfg in bad:
        assert lib.abnn_propagate_host(C.byref(cfg), n_nrn, 0.8, None, 0, x.ctypes.data, out.ctypes.data) == 1
        assert lib.abnn_propagate_rescale_host(C.byref(cfg), n_nrn, out.ctypes.data, x.ctypes.data, None) == 1


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_host_rule_equals_the_numpy_reference_word_for_word(seed):
    from abnn_amd import propagate as P

    n_nrn = 700 + seed
    syn = _records(20_000, seed, n_nrn)
    x = _x(n_nrn, seed)
    for k, cfg in enumerate(_configs(n_nrn)):
        base_scale = (0.8, 1.0, 3.5e4)[k % 3]  # the last one makes large coefficients: not summable ones too
        want = P.reference(syn, cfg, n_nrn, x, base_scale)
        got = P.host(syn, cfg, n_nrn, x, base_scale)
        assert np.array_equal(got, P.to_words(want)), (k, np.flatnonzero(got != P.to_words(want))[:8])
        d = P.decode(got, cfg, n_nrn)
        assert d["records"] == 20_000 and d["tombstones"] == int((syn["dst"] == NONE).sum())
        if k == 0:
            assert d["followed"] > 5_000 and 0 < d["skipped"] < d["followed"]
        x1, row = P.rescale_host(got, cfg, n_nrn, x)
        want_x, want_row = P.rescale_reference(want, cfg, n_nrn, x)
        assert np.array_equal(x1, want_x) and np.array_equal(row, want_row), k
        o0, oc = P.ranges(cfg, n_nrn)[2:]
        outside = np.ones(n_nrn, bool)
        outside[o0:o0 + oc] = False
        assert np.array_equal(x1[outside], x[outside])  # x outside the out-range is not touched
        if row[3]:
            m = int(np.abs(x1[o0:o0 + oc].astype(np.int64)).max())
            assert (1 << 29) <= m <= (1 << 30)


def test_rescale_edges():
    from abnn_amd import propagate as P

    cfg = P.config()
    x = np.full(4, 7, dtype=np.int32)
    for y, e in (([0, 0, 0, 0], 0), ([1, 0, 0, 0], 29), ([-1, 0, 0, 0], 29), ([(1 << 30) - 1, 5, 0, 0], 0),
                 ([1 << 30, -3, 0, 0], -1), ([-(1 << 63), (1 << 63) - 1, 1 << 34, -1], -34), ([(1 << 62) - 1, -(1 << 62), 0, 0], -33)):
        d = {"records": 0, "tombstones": 0, "followed": 3, "skipped": 1, "nnz": 2, "sum_abs_x": 9, "y": np.array(y, dtype=np.int64)}
        x1, row = P.rescale_host(P.to_words(d), cfg, 4, x)
        want_x, want_row = P.rescale_reference(d, cfg, 4, x)
        assert np.array_equal(x1, want_x) and np.array_equal(row, want_row), y
        assert int(row.view(np.int64)[4]) == e, (y, row)
        assert row[:2].tolist() == [2, 9] and row[5:].tolist() == [3, 1, 0]
        assert int(row[3]) == max(abs(v) for v in y) and int(row[2]) == sum(abs(v) for v in y) % (1 << 64)
        want = [v << e if e >= 0 else v >> -e for v in y]  # Python's shifts are arithmetic
        assert x1.tolist() == want, (y, x1.tolist())


def _ring(n, w):
    from abnn_amd import SYN_DTYPE

    syn = np.zeros(n, dtype=SYN_DTYPE)
    syn["src"] = np.arange(n)
    syn["dst"] = (np.arange(n) + 1) % n
    syn["w"] = w
    return syn


def test_a_directed_ring_halves_a_one_hot_at_every_step():
    from abnn_amd import propagate as P

    n = 37
    syn = _ring(n, 0.5)
    cfg = P.config()
    x = np.zeros(n, dtype=np.int32)
    x[3] = 1 << 30
    for step in range(1, 6):
        d = P.decode(P.host(syn, cfg, n, x), cfg, n)
        assert d["followed"] == 1 and d["nnz"] == 1 and d["sum_abs_x"] == int(np.abs(x.astype(np.int64)).sum())
        want = np.zeros(n, dtype=np.int64)
        want[(3 + step) % n] = (1 << 37) if step == 1 else (1 << 36)
        assert np.array_equal(d["y"], want)
        x, row = P.rescale_host(P.to_words(d), cfg, n, x)
        b = P.branching(row)
        assert b["ratio"] == 0.5 and int(b["e"][0]) == (-8 if step == 1 else -7)
        assert x[(3 + step) % n] == 1 << 29 and int(np.count_nonzero(x)) == 1
    xr, trace = P.iterate_reference(syn, cfg, n, np.where(np.arange(n) == 3, 1 << 30, 0), 5)
    assert np.array_equal(xr, x) and P.branching(trace)["estimates"].tolist() == [0.5] * 5
    # the transpose walks the ring backwards
    back = P.decode(P.host(syn, P.config(reverse=True), n, xr), P.config(reverse=True), n)
    assert np.flatnonzero(back["y"]).tolist() == [(3 + 4) % n]


def test_a_regular_graph_with_equal_weights_has_ratio_k_w():
    from abnn_amd import SYN_DTYPE
    from abnn_amd import propagate as P

    n, k, w = 64, 5, 0.25
    syn = np.zeros(n * k, dtype=SYN_DTYPE)
    syn["src"] = np.repeat(np.arange(n), k)
    syn["dst"] = (syn["src"] + np.tile(np.arange(1, k + 1), n)) % n  # every neuron: k out, k in
    syn["w"] = w
    cfg = P.config()
    x, trace = P.iterate_reference(syn, cfg, n, np.full(n, P.ONE >> 1, dtype=np.int32), 4)
    assert P.branching(trace)["estimates"].tolist() == [k * w] * 4 and len(set(x.tolist())) == 1
    xh = np.full(n, P.ONE >> 1, dtype=np.int32)
    for row in trace:
        xh, got = P.rescale_host(P.host(syn, cfg, n, xh), cfg, n, xh)
        assert np.array_equal(got, row)
    assert np.array_equal(xh, x)


def test_fire_p_takes_the_truncation_of_the_fp32_product():
    from abnn_amd import propagate as P

    syn = _ring(2, 0.5)
    c = F32(F32(0.5) * F32(0.5)) * F32(0.8)  # 0.2f
    q = int(np.float64(c) * (1 << 24))       # exact in double, truncated
    assert q == int(F32(0.2) * F32(16777216.0)) == 3355443
    x = np.array([1 << 16, -(1 << 16)], dtype=np.int32)  # term = q * x >> 16 = +-q
    d = P.decode(P.host(syn, P.config(fire_p=True), 2, x, 0.8), P.config(fire_p=True), 2)
    assert d["y"].tolist() == [-q, q] and d["skipped"] == 0
    assert np.array_equal(P.reference(syn, P.config(fire_p=True), 2, x, 0.8)["y"], d["y"])
    x = np.array([3, -3], dtype=np.int32)  # the shift is a floor
    d = P.decode(P.host(syn, P.config(fire_p=True), 2, x, 0.8), P.config(fire_p=True), 2)
    assert d["y"].tolist() == [(q * -3) >> 16, (q * 3) >> 16]


def test_merge_of_three_slices_equals_the_whole():
    from abnn_amd import propagate as P

    n_nrn = 500
    syn = _records(9_001, 5, n_nrn)
    syn["w"][::2] = 127.5  # large terms: the 64-bit sums wrap
    x = _x(n_nrn, 6, 0.1)
    x[::3] = I32_MIN
    for cfg in (P.config(), P.config(reverse=True, outputs=(100, 50)), P.config(fire_p=True, weights=(-1.0, 1.0))):
        whole = P.reference(syn, cfg, n_nrn, x, 0.8)
        parts = [P.decode(P.host(syn[lo:hi], cfg, n_nrn, x, 0.8), cfg, n_nrn) for lo, hi in ((0, 3000), (3000, 3001), (3001, 9001))]
        assert np.array_equal(P.to_words(P.merge(parts)), P.to_words(whole))
    with pytest.raises(ValueError):
        P.merge([whole, dict(whole, nnz=whole["nnz"] + 1)])


def test_fixed_point_helpers():
    from abnn_amd import propagate as P

    a = np.array([0.0, 1.0, -1.0, 0.5, 3.0, -3.0, 2.0 ** -30])
    v = P.to_fixed(a)
    assert v.dtype == np.int32 and v.tolist() == [0, 1 << 30, -(1 << 30), 1 << 29, I32_MAX, I32_MIN, 1]
    assert P.from_fixed(v[:4]).tolist() == [0.0, 1.0, -1.0, 0.5]
    assert P.from_fixed(np.array([1 << 38], dtype=np.int64), frac_bits=P.Y_FRAC_BITS).tolist() == [1.0]


def test_config_layout_matches_c(tmp_path):
    from abnn_amd import _lib

    fields = ["in_first", "in_count", "out_first", "out_count", "flags", "w_lo", "w_hi", "reserved"]
    prog = tmp_path / "sz.c"
    prog.write_text('#include "abnn/abnn.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                    'int main(void){printf("%zu", sizeof(abnn_propagate_config));\n' +
                    "".join(f'printf(" %zu", offsetof(abnn_propagate_config, {f}));\n' for f in fields) +
                    'printf(" %u %u %u %u %u %u\\n", ABNN_PROP_REVERSE, ABNN_PROP_FIRE_P, ABNN_PROP_WEIGHT,'
                    'ABNN_PROP_HEADER_WORDS, ABNN_PROP_TRACE_WORDS, ABNN_PROP_MAX_STEPS);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(_lib.PropagateConfig)] + [getattr(_lib.PropagateConfig, f).offset for f in fields] + \
        [_lib.PROP_REVERSE, _lib.PROP_FIRE_P, _lib.PROP_WEIGHT, _lib.PROP_HEADER_WORDS, _lib.PROP_TRACE_WORDS,
         _lib.PROP_MAX_STEPS]
    assert got == want and got[0] == 48
