"""CPU checks of the reachability search's boundary (abnn.h abnn_hops_*): the
ctypes mirror matches the C layout, abnn_hops_words against hops.n_words on
valid and invalid configs, null handles without a GPU, and the numpy
restatement (abnn_amd.hops.reference / step / merge_planes) on a hand-made
record array whose levels and planes are written out by hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NONE = 0xFFFFFFFF
U = 0xFFFFFFFF  # ABNN_HOPS_UNREACHED
SYN = [("src", "<u4"), ("dst", "<u4"), ("w", "<f4"), ("pad", "<f4")]


def test_hops_config_layout_matches_c(tmp_path):
    from abnn_amd import _lib

    fields = [n for n, _ in _lib.HopsConfig._fields_]
    prog = tmp_path / "sz.c"
    prog.write_text('#include "abnn/abnn.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                    'int main(void){printf("%zu %d %u %u %u %u %u", sizeof(abnn_hops_config), ABNN_HOPS_HEADER_WORDS,'
                    ' ABNN_HOPS_MAX, ABNN_HOPS_REVERSE, ABNN_HOPS_WEIGHT, ABNN_HOPS_UNREACHED, ABNN_HOPS_BEGIN);\n'
                    + "".join(f'printf(" %zu", offsetof(abnn_hops_config, {f}));\n' for f in fields)
                    + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(_lib.HopsConfig), _lib.HOPS_HEADER_WORDS, _lib.HOPS_MAX, _lib.HOPS_REVERSE, _lib.HOPS_WEIGHT,
            _lib.HOPS_UNREACHED, _lib.HOPS_BEGIN, *(getattr(_lib.HopsConfig, f).offset for f in fields)]
    assert got == want
    assert got[:7] == [32, 8, 1024, 1, 2, 0xFFFFFFFF, 0xFFFFFFFF]
    assert got[7:] == [0, 4, 8, 12, 16, 20, 24]
    assert fields == ["seed_first", "seed_count", "max_hops", "flags", "w_lo", "w_hi", "reserved"]


def test_fold_constants_mirror_the_header():
    import re

    from abnn_amd import hops

    with open(os.path.join(ROOT, "abnn_amd", "csrc", "hops.h")) as f:
        text = f.read()
    m = re.search(r"kHopsFoldWords\s*=\s*(\d+)\s*;", text)
    assert m and int(m.group(1)) == hops.FOLD_WORDS
    assert re.search(r"kHopsFoldMaxFrontier\s*=\s*32\s*\*\s*kHopsFoldWords\s*/\s*8\s*;", text)
    assert hops.FOLD_MAX_FRONTIER == 32 * hops.FOLD_WORDS // 8 == 32_768


def _invalid_configs():
    """name -> (config, n_nrn): every refusal abnn.h lists that needs no handle (null is checked apart)."""
    from abnn_amd import hops

    bad = {
        "seed_count 0": (hops.config((5, 0)), 1000),
        "seed range ends above n_nrn": (hops.config((900, 101)), 1000),
        "seed_first above n_nrn": (hops.config((1001, 1)), 1000),
        "seed range wraps u32": (hops.config((0xFFFFFFFF, 2)), 1000),
        "max_hops 0": (hops.config((0, 1), 0), 1000),
        "max_hops 1025": (hops.config((0, 1), 1025), 1000),
        "n_nrn 0": (hops.config((0, 1)), 0),
        "w_lo without WEIGHT": (hops.config((0, 1)), 1000),
        "w_hi without WEIGHT": (hops.config((0, 1)), 1000),
        "-0.0 without WEIGHT": (hops.config((0, 1)), 1000),
        "NaN w_lo": (hops.config((0, 1), weights=(np.nan, 1.0)), 1000),
        "NaN w_hi": (hops.config((0, 1), weights=(0.0, np.nan)), 1000),
        "w_lo == w_hi": (hops.config((0, 1), weights=(0.5, 0.5)), 1000),
        "w_lo > w_hi": (hops.config((0, 1), weights=(0.5, 0.25)), 1000),
    }
    bad["w_lo without WEIGHT"][0].w_lo = 0.5
    bad["w_hi without WEIGHT"][0].w_hi = 0.5
    bad["-0.0 without WEIGHT"][0].w_lo = -0.0
    for bit in (4, 8, 1 << 31):
        cfg = hops.config((0, 1), reverse=True)
        cfg.flags |= bit
        bad[f"flag bit {bit}"] = (cfg, 1000)
    for k in range(2):
        cfg = hops.config((0, 10))
        cfg.reserved[k] = 1
        bad[f"reserved[{k}]"] = (cfg, 1000)
    return bad


def test_hops_words():
    from abnn_amd import _lib, hops

    lib = _lib.load()
    empty = np.zeros(0, dtype=SYN)
    for n_nrn in (1000, 5_000_512, 1001):
        for H in (1, 64, 1024):
            for seeds in ((0, 1), (n_nrn - 1, 1), (256, 256), (0, n_nrn)):
                for reverse in (False, True):
                    for weights in (None, (0.25, 0.9), (-np.inf, np.inf)):
                        cfg = hops.config(seeds, H, reverse, weights)
                        want = 8 + (H + 1) + (n_nrn + 1) // 2
                        assert lib.abnn_hops_words(C.byref(cfg), n_nrn) == want == hops.n_words(cfg, n_nrn), (n_nrn, H, seeds)
    assert hops.n_words(hops.config((0, 1)), 5_000_512) == 8 + 65 + 2_500_256  # the default H is 64
    for name, (cfg, n_nrn) in _invalid_configs().items():
        assert lib.abnn_hops_words(C.byref(cfg), n_nrn) == 0, name
        assert hops.n_words(cfg, n_nrn) == 0, name
        with pytest.raises(ValueError):
            hops.reference(empty, cfg, n_nrn)
    assert lib.abnn_hops_words(None, 1000) == 0
    cfg = hops.config((3, 4), 7, reverse=True, weights=(0.25, 0.5))
    assert (cfg.seed_first, cfg.seed_count, cfg.max_hops, cfg.flags, cfg.w_lo, cfg.w_hi) == (3, 4, 7, 3, 0.25, 0.5)
    assert hops.config((3, 4)).flags == 0 and hops.config((3, 4)).max_hops == 64
    assert hops.BEGIN == 0xFFFFFFFF == hops.UNREACHED


def test_hops_null_arguments_are_invalid_without_a_gpu():
    from abnn_amd import _lib, hops

    lib = _lib.load()
    cfg = hops.config((0, 4), 2)
    words = hops.n_words(cfg, 10)
    out = (C.c_uint64 * words)()
    assert lib.abnn_hops_enqueue(None, C.byref(cfg), out, None) == 1  # ABNN_ERR_INVALID
    assert lib.abnn_hops_step_enqueue(None, C.byref(cfg), hops.BEGIN, out, None) == 1
    assert lib.abnn_hops_step_enqueue(None, C.byref(cfg), 0, out, None) == 1
    assert lib.abnn_hops(None, C.byref(cfg), out, words) == 1
    assert lib.abnn_hops(None, None, None, 0) == 1


N_NRN = 10


def _hand_made():
    """15 records over 10 neurons: a branch, a cycle, a self-loop, a duplicate
    edge, a tombstone, a NaN weight, a weight exactly at w_hi = 0.9, an edge
    into the seed, and two records that point outside the planes."""
    rec = [
        (0, 1, 0.5),        # 0  the branch out of neuron 0 ...
        (0, 2, 0.5),        # 1  ... its other arm
        (1, 3, 0.5),        # 2  both arms meet in 3
        (2, 3, 0.5),        # 3
        (3, 4, 0.5),        # 4  the cycle 3 -> 4 -> 5 -> 3
        (4, 5, 0.5),        # 5
        (5, 3, 0.5),        # 6  closes the cycle: 3 keeps its distance
        (4, 4, 0.5),        # 7  a self-loop
        (0, 1, 0.6),        # 8  a duplicate edge
        (NONE, NONE, 0.5),  # 9  a tombstone
        (5, 6, np.nan),     # 10 followed unless a weight interval is asked
        (5, 7, 0.9),        # 11 exactly w_hi: outside [0.25, 0.9)
        (8, 0, 0.5),        # 12 into the seed: matters in reverse only
        (3, 10, 0.5),       # 13 dst == N_NRN: never followed
        (10, 9, 0.5),       # 14 src == N_NRN: never followed, 9 stays unreached
    ]
    syn = np.zeros(len(rec), dtype=SYN)
    for k, (s, d, w) in enumerate(rec):
        syn[k] = (s, d, F32(w), 0.0)
    return syn


# (seeds, H, reverse, weights) -> levels, dist, reached, depth, complete: worked out by hand
HAND = [
    (((0, 1), 8, False, None), [1, 2, 1, 1, 1, 2, 0, 0, 0], [0, 1, 1, 2, 3, 4, 5, 5, U, U], 8, 5, 1),
    (((0, 1), 8, False, (0.25, 0.9)), [1, 2, 1, 1, 1, 0, 0, 0, 0], [0, 1, 1, 2, 3, 4, U, U, U, U], 6, 4, 1),
    (((0, 1), 3, False, None), [1, 2, 1, 1], [0, 1, 1, 2, 3, U, U, U, U, U], 5, 3, 0),
    (((0, 1), 5, False, None), [1, 2, 1, 1, 1, 2], [0, 1, 1, 2, 3, 4, 5, 5, U, U], 8, 5, 0),  # levels[H] > 0
    (((7, 1), 8, True, None), [1, 1, 1, 1, 2, 1, 1, 0, 0], [5, 4, 4, 3, 2, 1, U, 0, 6, U], 8, 6, 1),
    (((7, 1), 8, True, (0.25, 0.9)), [1, 0, 0, 0, 0, 0, 0, 0, 0], [U, U, U, U, U, U, U, 0, U, U], 1, 0, 1),
    (((6, 2), 2, True, None), [2, 1, 1], [U, U, U, U, 2, 1, 0, 0, U, U], 4, 2, 0),
    (((3, 3), 1, False, (0.5, np.inf)), [3, 1], [U, U, U, 0, 0, 0, U, 1, U, U], 4, 1, 0),  # NaN is not followed
]


@pytest.mark.parametrize("case", range(len(HAND)))
def test_reference_known_answer(case):
    from abnn_amd import hops

    args, levels, dist, reached, depth, complete = HAND[case]
    syn = _hand_made()
    cfg = hops.config(*args)
    got = hops.reference(syn, cfg, N_NRN)
    assert got["levels"].tolist() == levels and got["dist"].tolist() == dist
    assert (got["records"], got["neurons"], got["reached"], got["depth"], got["complete"]) == (15, N_NRN, reached, depth, complete)
    assert got["levels"].dtype == np.uint64 and got["dist"].dtype == np.uint32
    assert got["reached"] == int((got["dist"] != U).sum()) == sum(levels)
    # the words and back
    words = hops.to_words(got)
    assert words.dtype == np.uint64 and words.shape == (hops.n_words(cfg, N_NRN),)
    assert words[:8].tolist() == [15, N_NRN, reached, depth, complete, 0, 0, 0]
    assert words[8:8 + len(levels)].tolist() == levels
    back = hops.decode(words, cfg, N_NRN)
    assert set(back) == set(got)
    for k, v in got.items():
        assert np.array_equal(back[k], v) and np.asarray(back[k]).dtype == np.asarray(v).dtype, k


def test_reference_edges():
    from abnn_amd import hops

    syn = _hand_made()
    # no records: the seeds only
    none = hops.reference(syn[:0], hops.config((2, 3), 4), N_NRN)
    assert none["levels"].tolist() == [3, 0, 0, 0, 0] and none["reached"] == 3 and none["complete"] == 1
    assert none["dist"].tolist() == [U, U, 0, 0, 0, U, U, U, U, U] and none["records"] == 0
    # an odd N_NRN: the plane is padded with one zero entry
    odd = hops.reference(syn[:9], hops.config((0, 1), 2), 9)
    words = hops.to_words(odd)
    assert words.shape == (8 + 3 + 5,) and int(words[-1]) >> 32 == 0 and int(words[-1]) & 0xFFFFFFFF == U
    assert np.array_equal(hops.decode(words, hops.config((0, 1), 2), 9)["dist"], odd["dist"])
    # every neuron a seed
    full = hops.reference(syn, hops.config((0, N_NRN), 1), N_NRN)
    assert full["levels"].tolist() == [N_NRN, 0] and full["depth"] == 0 and not full["dist"].any()


@pytest.mark.parametrize("case", range(len(HAND)))
def test_merge_planes_of_a_stepped_three_way_split(case):
    from abnn_amd import hops

    args = HAND[case][0]
    syn = _hand_made()
    cfg = hops.config(*args)
    whole = hops.reference(syn, cfg, N_NRN)
    parts = [syn[a:b] for a, b in ((0, 5), (5, 9), (9, 15))]
    uv = [hops.edges(p, cfg, N_NRN) for p in parts]
    state = [hops.begin(cfg, N_NRN) for _ in parts]
    for h in range(cfg.max_hops + 1):
        for e, (levels, plane) in zip(uv, state):
            hops.step(e, cfg, levels, plane, h)
        merged = hops.merge_planes([plane for _, plane in state])
        for _, plane in state:
            plane[:] = merged
    for p, (levels, plane) in zip(parts, state):
        got = hops.close(cfg, levels, plane, len(p))
        assert got["records"] == len(p)
        got["records"] = whole["records"]
        assert np.array_equal(hops.to_words(got), hops.to_words(whole))
    # one part alone does not see the whole graph
    if case == 0:
        alone = hops.reference(parts[0], cfg, N_NRN)
        assert alone["reached"] < whole["reached"]
    assert hops.merge_planes([np.array([3, U, 0], dtype=np.uint32), np.array([U, U, 7], dtype=np.uint32)]).tolist() == [3, U, 0]
    with pytest.raises(ValueError):
        hops.merge_planes([])
    with pytest.raises(ValueError):
        hops.merge_planes([np.zeros(3, dtype=np.uint32), np.zeros(4, dtype=np.uint32)])
