"""CPU checks of the synapse census's boundary (abnn.h abnn_census_*,
abnn_engine_*_census): the ctypes mirror matches the C layout, the config
validation, null handles without a GPU, and the numpy restatement
(abnn_amd.census.reference / merge) on a hand-made record array whose result
is written out by hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NONE = 0xFFFFFFFF


def test_census_config_layout_matches_c(tmp_path):
    from abnn_amd import _lib

    fields = [n for n, _ in _lib.CensusConfig._fields_]
    prog = tmp_path / "sz.c"
    prog.write_text('#include "abnn/abnn.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                    'int main(void){printf("%zu %d %d", sizeof(abnn_census_config), ABNN_CENSUS_HEADER_WORDS,'
                    ' ABNN_CENSUS_MAX_BINS);\n'
                    + "".join(f'printf(" %zu", offsetof(abnn_census_config, {f}));\n' for f in fields)
                    + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(_lib.CensusConfig), _lib.CENSUS_HEADER_WORDS, _lib.CENSUS_MAX_BINS,
            *(getattr(_lib.CensusConfig, f).offset for f in fields)]
    assert got == want
    assert got[:3] == [32, 8, 4096]
    assert fields == ["lo", "hi", "bins", "src_first", "src_count", "dst_first", "dst_count", "reserved"]


def _invalid_configs():
    from abnn_amd import census

    bad = {
        "bins 0": census.config(0, 0.0, 1.0),
        "bins above 4096": census.config(4097, 0.0, 1.0),
        "lo == hi": census.config(8, 0.5, 0.5),
        "lo > hi": census.config(8, 1.0, 0.0),
        "lo nan": census.config(8, float("nan"), 1.0),
        "hi nan": census.config(8, 0.0, float("nan")),
        "lo -inf": census.config(8, float("-inf"), 1.0),
        "hi inf": census.config(8, 0.0, float("inf")),
        "scale overflows": census.config(4096, 0.0, 1e-40),
        "reserved": census.config(8, 0.0, 1.0),
    }
    bad["reserved"].reserved = 1
    return bad


def test_census_words():
    from abnn_amd import _lib, census

    lib = _lib.load()
    for bins in (1, 7, 64, 4096):
        for lo, hi in ((0.0, 1.0), (-0.1, 1.1), (-3.0e38, -1.0e38), (1e-30, 2e-30)):
            cfg = census.config(bins, lo, hi, src=(5, 10), dst=(0, 0))
            assert lib.abnn_census_words(C.byref(cfg)) == 8 + bins == census.n_words(cfg), (bins, lo, hi)
    for name, cfg in _invalid_configs().items():
        assert lib.abnn_census_words(C.byref(cfg)) == 0, name
        assert census.n_words(cfg) == 0, name
        with pytest.raises(ValueError):
            census.reference(np.zeros(0, dtype=[("src", "<u4"), ("dst", "<u4"), ("w", "<f4"), ("pad", "<f4")]), cfg)
    assert lib.abnn_census_words(None) == 0


def test_census_null_handles_are_invalid_without_a_gpu():
    from abnn_amd import _lib, census

    lib = _lib.load()
    cfg = census.config(64, 0.0, 1.0)
    out = (C.c_uint64 * 72)()
    assert lib.abnn_census_enqueue(None, C.byref(cfg), out, None) == 1  # ABNN_ERR_INVALID
    assert lib.abnn_census(None, C.byref(cfg), out, 72) == 1
    assert lib.abnn_engine_set_census(None, C.byref(cfg), 1, 1) == 1
    assert lib.abnn_engine_set_census(None, None, 0, 0) == 1
    assert lib.abnn_engine_census_count(None) == 0
    steps = (C.c_uint64 * 1)()
    assert lib.abnn_engine_read_census(None, 0, 1, out, steps) == 1
    assert lib.abnn_engine_read_census(None, 0, 0, None, None) == 1


def hand_made_records():
    """40 records: the bin edges, the non-finite values, both zeros, two
    tombstones, then 30 weights 1/64 + k/32 (k = 0..29: bin k // 4 of 8 over [0, 1))."""
    from abnn_amd import SYN_DTYPE

    syn = np.zeros(40, dtype=SYN_DTYPE)
    head = [(1, 600, 0.0),                              # exactly lo
            (2, 601, np.nextafter(F32(1), F32(0))),     # the largest float below hi
            (3, 602, 1.0),                              # exactly hi
            (4, 603, -0.25),                            # below lo
            (5, 604, np.inf), (6, 605, -np.inf), (7, 606, np.nan),
            (1, 607, -0.0),
            (NONE, NONE, 0.3), (NONE, NONE, np.nan)]    # tombstones (a NaN weight is not counted)
    for i, (s, d, w) in enumerate(head):
        syn[i] = (s, d, w, 0)
    for i in range(10, 40):
        syn[i] = (100 + i, 700 + i % 10, F32(1 / 64) + F32(i - 10) / F32(32), 0)
    return syn


def _bits(x):
    return int(np.array([x], dtype=F32).view(np.uint32)[0])


def _scalar_census(syn, cfg):
    """abnn.h's definition one record at a time (independent of census.reference's vector form)."""
    lo, hi, bins = F32(cfg.lo), F32(cfg.hi), cfg.bins
    scale = F32(bins) / (hi - lo)
    key = lambda b: (b ^ 0xFFFFFFFF) if b >> 31 else (b | 0x80000000)
    r = dict(records=len(syn), tombstones=0, selected=0, under=0, over=0, nan=0)
    counts, kmin, kmax = [0] * bins, None, None
    for s, d, w, _ in syn.tolist():
        if d == NONE:
            r["tombstones"] += 1
            continue
        if cfg.src_count and not cfg.src_first <= s < cfg.src_first + cfg.src_count:
            continue
        if cfg.dst_count and not cfg.dst_first <= d < cfg.dst_first + cfg.dst_count:
            continue
        r["selected"] += 1
        w = F32(w)
        if w != w:
            r["nan"] += 1
            continue
        k = key(_bits(w))
        kmin, kmax = (k if kmin is None else min(k, kmin)), (k if kmax is None else max(k, kmax))
        if w < lo:
            r["under"] += 1
        elif w >= hi:
            r["over"] += 1
        else:
            counts[min(int(F32(F32(w - lo) * scale)), bins - 1)] += 1
    unkey = lambda k: (k ^ 0x80000000) if k >> 31 else (k ^ 0xFFFFFFFF)
    r["min_bits"] = 0x7F800000 if kmin is None else unkey(kmin)
    r["max_bits"] = 0xFF800000 if kmax is None else unkey(kmax)
    r["counts"] = counts
    return r


def _check(got, want):
    for k in ("records", "tombstones", "selected", "under", "over", "nan"):
        assert got[k] == want[k], k
    assert got["live"] == want["records"] - want["tombstones"]
    assert _bits(got["min"]) == want["min_bits"] and _bits(got["max"]) == want["max_bits"]
    assert got["counts"].dtype == np.uint64 and got["counts"].tolist() == want["counts"]
    assert got["selected"] == got["under"] + got["over"] + got["nan"] + int(got["counts"].sum())
    assert len(got["edges"]) == len(want["counts"]) + 1


INF, NINF = 0x7F800000, 0xFF800000

# (bins, lo, hi, src, dst) -> the result, worked out by hand from hand_made_records
HAND_CASES = [
    ((8, 0.0, 1.0, None, None),
     dict(records=40, tombstones=2, selected=38, under=2, over=2, nan=1, min_bits=NINF, max_bits=INF,
          counts=[6, 4, 4, 4, 4, 4, 4, 3])),      # bin 0: +0.0, -0.0, k = 0..3; bin 7: k = 28, 29 and 1 - ulp
    ((1, 0.0, 1.0, None, None),
     dict(records=40, tombstones=2, selected=38, under=2, over=2, nan=1, min_bits=NINF, max_bits=INF, counts=[33])),
    ((8, 0.0, 1.0, (1, 8), None),                  # the eight special records
     dict(records=40, tombstones=2, selected=8, under=2, over=2, nan=1, min_bits=NINF, max_bits=INF,
          counts=[2, 0, 0, 0, 0, 0, 0, 1])),
    ((8, 0.0, 1.0, None, (700, 5)),                # k = 0..4, 10..14, 20..24
     dict(records=40, tombstones=2, selected=15, under=0, over=0, nan=0, min_bits=_bits(1 / 64),
          max_bits=_bits(24 / 32 + 1 / 64), counts=[4, 1, 2, 3, 0, 4, 1, 0])),
    ((8, 0.0, 1.0, (110, 10), (700, 5)),           # both ranges: k = 0..4
     dict(records=40, tombstones=2, selected=5, under=0, over=0, nan=0, min_bits=_bits(1 / 64),
          max_bits=_bits(4 / 32 + 1 / 64), counts=[4, 1, 0, 0, 0, 0, 0, 0])),
    ((8, 0.0, 1.0, (1, 1), None),                  # +0.0 and -0.0: both bin 0, -0.0 is the minimum
     dict(records=40, tombstones=2, selected=2, under=0, over=0, nan=0, min_bits=0x80000000, max_bits=0,
          counts=[2, 0, 0, 0, 0, 0, 0, 0])),
    ((8, 0.0, 1.0, (900, 10), None),               # nothing selected
     dict(records=40, tombstones=2, selected=0, under=0, over=0, nan=0, min_bits=INF, max_bits=NINF, counts=[0] * 8)),
]


@pytest.mark.parametrize("args,want", HAND_CASES, ids=[str(i) for i in range(len(HAND_CASES))])
def test_reference_on_hand_made_records(args, want):
    from abnn_amd import census

    syn = hand_made_records()
    cfg = census.config(*args)
    assert _scalar_census(syn, cfg) == want
    _check(census.reference(syn, cfg), want)


@pytest.mark.parametrize("args", [(7, 0.0, 1.0, None, None), (64, -0.1, 1.1, None, None),
                                  (4096, 0.25, 0.75, None, (700, 8)), (4096, 0.0, 1.0, (1, 200), None)])
def test_reference_equals_the_scalar_restatement(args):
    from abnn_amd import census

    syn = hand_made_records()
    cfg = census.config(*args)
    _check(census.reference(syn, cfg), _scalar_census(syn, cfg))


def test_merge_of_a_three_way_split_equals_the_whole():
    from abnn_amd import census

    syn = hand_made_records()
    for args, _ in HAND_CASES:
        cfg = census.config(*args)
        whole = census.reference(syn, cfg)
        for cuts in ((13, 14), (3, 9), (0, 40), (7, 8)):
            parts = [census.reference(p, cfg) for p in np.split(syn, cuts)]
            merged = census.merge(parts)
            assert np.array_equal(census.to_words(merged), census.to_words(whole)), (args, cuts)
            assert merged["live"] == whole["live"] and np.array_equal(merged["edges"], whole["edges"])
    # words round-trip through decode
    cfg = census.config(8, 0.0, 1.0)
    words = census.to_words(census.reference(syn, cfg))
    assert words.dtype == np.uint64 and words.shape == (16,)
    assert np.array_equal(census.to_words(census.decode(words, cfg)), words)
    with pytest.raises(ValueError):
        census.merge([])
