"""CPU checks of the neuron degree census's boundary (abnn.h abnn_degree_*):
the ctypes mirror matches the C layout, abnn_degree_words against
degree.n_words on valid and invalid configs, null handles without a GPU, and
the numpy restatement (abnn_amd.degree.reference / merge) on a hand-made record
array whose result is written out by hand."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NONE = 0xFFFFFFFF
SYN = [("src", "<u4"), ("dst", "<u4"), ("w", "<f4"), ("pad", "<f4")]


def test_degree_config_layout_matches_c(tmp_path):
    from abnn_amd import _lib

    fields = [n for n, _ in _lib.DegreeConfig._fields_]
    prog = tmp_path / "sz.c"
    prog.write_text('#include "abnn/abnn.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                    'int main(void){printf("%zu %d %u %u %u %u", sizeof(abnn_degree_config), ABNN_DEGREE_HEADER_WORDS,'
                    ' ABNN_DEG_OUT, ABNN_DEG_IN, ABNN_DEG_OUT_W, ABNN_DEG_IN_W);\n'
                    + "".join(f'printf(" %zu", offsetof(abnn_degree_config, {f}));\n' for f in fields)
                    + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(_lib.DegreeConfig), _lib.DEGREE_HEADER_WORDS, _lib.DEG_OUT, _lib.DEG_IN, _lib.DEG_OUT_W,
            _lib.DEG_IN_W, *(getattr(_lib.DegreeConfig, f).offset for f in fields)]
    assert got == want
    assert got[:6] == [32, 8, 1, 2, 4, 8]
    assert fields == ["first", "count", "what", "reserved"]


def test_narrow_max_mirrors_the_header():
    from abnn_amd import degree

    with open(os.path.join(ROOT, "abnn_amd", "csrc", "degree.h")) as f:
        text = f.read()
    m = re.search(r"kDegreeNarrowMax\s*=\s*(\d+)\s*;", text)
    assert m and int(m.group(1)) == degree.NARROW_MAX
    m = re.search(r"kDegreeLdsBytes\s*=\s*(\d+)\s*\*\s*(\d+)\s*;", text)
    assert m and int(m.group(1)) * int(m.group(2)) == degree.NARROW_LDS_BYTES


def _invalid_configs():
    """name -> (config, n_nrn): every refusal abnn.h lists (null is checked apart)."""
    from abnn_amd import degree

    bad = {
        "what 0": (degree.config(None, 0), 1000),
        "what bit 4": (degree.config(None, 16), 1000),
        "what bit 4 with valid bits": (degree.config((0, 10), 15 | 32), 1000),
        "count 0 with first != 0": (degree.config((5, 0), 15), 1000),
        "range ends above n_nrn": (degree.config((900, 101), 15), 1000),
        "first above n_nrn": (degree.config((1001, 1), 1), 1000),
        "first + count wraps u32": (degree.config((0xFFFFFFFF, 2), 1), 1000),
        "n_nrn 0": (degree.config(None, 15), 0),
        "n_nrn 0 with a range": (degree.config((0, 1), 15), 0),
    }
    for k in range(5):
        cfg = degree.config((0, 10), 15)
        cfg.reserved[k] = 1
        bad[f"reserved[{k}]"] = (cfg, 1000)
    return bad


def test_degree_words():
    from abnn_amd import _lib, degree

    lib = _lib.load()
    empty = np.zeros(0, dtype=SYN)
    for what in range(1, 16):
        planes = bin(what).count("1")
        for n_nrn in (1000, 5_000_512):
            for neurons, m in ((None, n_nrn), ((0, 1), 1), ((n_nrn - 1, 1), 1), ((256, 256), 256), ((0, n_nrn), n_nrn)):
                cfg = degree.config(neurons, what)
                want = 8 + planes * m
                assert lib.abnn_degree_words(C.byref(cfg), n_nrn) == want == degree.n_words(cfg, n_nrn), (what, neurons)
    assert {bin(w).count("1") for w in range(1, 16)} == {1, 2, 3, 4}
    assert degree.n_words(degree.config(None, 15), 5_000_512) == 8 + 4 * 5_000_512
    for name, (cfg, n_nrn) in _invalid_configs().items():
        assert lib.abnn_degree_words(C.byref(cfg), n_nrn) == 0, name
        assert degree.n_words(cfg, n_nrn) == 0, name
        with pytest.raises(ValueError):
            degree.reference(empty, cfg, n_nrn)
    assert lib.abnn_degree_words(None, 1000) == 0
    # plane names and bits are the same thing
    assert degree.config((1, 2), ("in", "out_w")).what == 2 | 4 and degree.config().what == 15
    assert degree.config(None, "in").what == 2
    with pytest.raises(ValueError):
        degree.config(None, ("inn",))


def test_degree_null_arguments_are_invalid_without_a_gpu():
    from abnn_amd import _lib, degree

    lib = _lib.load()
    cfg = degree.config((0, 4), 15)
    out = (C.c_uint64 * 24)()
    assert lib.abnn_degree_enqueue(None, C.byref(cfg), out, None) == 1  # ABNN_ERR_INVALID
    assert lib.abnn_degree(None, C.byref(cfg), out, 24) == 1
    assert lib.abnn_degree(None, None, None, 0) == 1


def _hand_made():
    """13 records over 10 neurons, R = neurons 2..5: a tombstone, three
    self-loops, src or dst or both outside R, and the special weights."""
    rec = [
        (2, 3, np.nan),          # 0  not summable: counted, skipped on both sides
        (3, 3, np.inf),          # 1  self-loop, not summable
        (2, 4, -0.0),            # 2  term 0
        (4, 2, 1e-40),           # 3  a denormal: term 0
        (5, 5, 127.99999),       # 4  self-loop, the largest summable float32: 2^31 - 2^7
        (2, 5, 128.0),           # 5  not summable
        (3, 2, -127.99999),      # 6
        (2, 9, 0.001),           # 7  dst outside R; 0.001f * 2^24 = 16777.2...
        (8, 3, 2.0 ** -24),      # 8  src outside R; term 1
        (NONE, NONE, 0.5),       # 9  tombstone
        (4, 4, 2.0 ** -25),      # 10 self-loop, term 0 (truncation)
        (5, 2, -(2.0 ** -24)),   # 11 term -1
        (0, 1, 0.5),             # 12 both outside R
    ]
    syn = np.zeros(len(rec), dtype=SYN)
    for k, (s, d, w) in enumerate(rec):
        syn[k] = (s, d, F32(w), 0.0)
    return syn


BIG = 2147483520  # (int32)(127.99999f * 2^24)
HAND_WANT = {
    "records": 13, "tombstones": 1, "out_total": 10, "in_total": 10, "out_skipped": 3, "in_skipped": 3,
    "first": 2, "count": 4,
    "out": [4, 2, 2, 2], "in": [3, 3, 2, 2],
    "out_w": [16777, -BIG, 0, BIG - 1], "in_w": [-BIG - 1, 1, 0, BIG],
}


def test_terms_of_the_special_weights():
    from abnn_amd import degree

    w = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-40, -1e-40, 127.99999, 128.0, -128.0, -127.99999, 0.001,
                  2.0 ** -24, 2.0 ** -25, -(2.0 ** -24)], dtype=F32)
    ok, q = degree.terms(w)
    assert ok.tolist() == [False, False, False, True, True, True, True, True, False, False, True, True, True, True, True]
    assert q.tolist() == [0, 0, 0, 0, 0, 0, 0, BIG, 0, 0, -BIG, 16777, 1, 0, -1]
    assert q.dtype == np.int64


def test_reference_known_answer():
    from abnn_amd import degree

    syn = _hand_made()
    got = degree.reference(syn, degree.config((2, 4), 15), 10)
    for k, want in HAND_WANT.items():
        if isinstance(want, list):
            assert got[k].tolist() == want, k
        else:
            assert got[k] == want, k
    assert got["out"].dtype == got["in"].dtype == np.uint64
    assert got["out_w"].dtype == got["in_w"].dtype == np.int64
    assert got["out_total"] == int(got["out"].sum()) and got["in_total"] == int(got["in"].sum())
    # a subset of the planes: the other side's words stay 0, the skipped word needs its strength plane
    one = degree.reference(syn, degree.config((2, 4), ("in",)), 10)
    assert set(one) & {"out", "in", "out_w", "in_w"} == {"in"} and one["in"].tolist() == HAND_WANT["in"]
    assert (one["out_total"], one["in_total"], one["out_skipped"], one["in_skipped"]) == (0, 10, 0, 0)
    only_w = degree.reference(syn, degree.config((2, 4), ("out_w",)), 10)
    assert set(only_w) & {"out", "in", "out_w", "in_w"} == {"out_w"} and only_w["out_w"].tolist() == HAND_WANT["out_w"]
    assert (only_w["out_total"], only_w["in_total"], only_w["out_skipped"], only_w["in_skipped"]) == (10, 0, 3, 0)
    # every neuron: the self-loops count on both sides, the tombstone on neither
    whole = degree.reference(syn, degree.config(None, 15), 10)
    assert whole["first"] == 0 and whole["count"] == 10
    assert whole["out_total"] == whole["in_total"] == 12 == whole["records"] - whole["tombstones"]
    assert whole["out"].tolist() == [1, 0, 4, 2, 2, 2, 0, 0, 1, 0] and whole["in"].tolist() == [0, 1, 3, 3, 2, 2, 0, 0, 0, 1]
    assert whole["out_w"][8] == 1 and whole["in_w"][9] == 16777 and whole["out_w"][0] == 1 << 23
    # no records at all
    none = degree.reference(syn[:0], degree.config((2, 4), 15), 10)
    assert degree.to_words(none).tolist() == [0] * 24


def test_decode_and_to_words_round_trip():
    from abnn_amd import degree

    syn = _hand_made()
    for neurons in ((2, 4), None, (9, 1)):
        for what in (15, 1, 2, 4, 8, 3, 12, 6):
            cfg = degree.config(neurons, what)
            d = degree.reference(syn, cfg, 10)
            words = degree.to_words(d)
            assert words.dtype == np.uint64 and words.shape == (degree.n_words(cfg, 10),)
            assert words[6] == 0 and words[7] == 0
            back = degree.decode(words, cfg, 10)
            assert set(back) == set(d)
            assert np.array_equal(degree.to_words(back), words)
            for k, v in d.items():
                assert np.array_equal(back[k], v) and np.asarray(back[k]).dtype == np.asarray(v).dtype, k
    # the planes follow the header in increasing bit order
    words = degree.to_words(degree.reference(syn, degree.config((2, 4), 15), 10))
    assert words[:6].tolist() == [13, 1, 10, 10, 3, 3]
    assert words[8:16].tolist() == HAND_WANT["out"] + HAND_WANT["in"]
    assert words[16:].view(np.int64).tolist() == HAND_WANT["out_w"] + HAND_WANT["in_w"]


def test_merge_of_a_three_way_split():
    from abnn_amd import degree

    syn = _hand_made()
    for neurons in ((2, 4), None):
        for what in (15, 2, 12):
            cfg = degree.config(neurons, what)
            parts = [degree.reference(syn[a:b], cfg, 10) for a, b in ((0, 5), (5, 9), (9, 13))]
            assert [p["records"] for p in parts] == [5, 4, 4]
            merged = degree.merge(parts)
            assert np.array_equal(degree.to_words(merged), degree.to_words(degree.reference(syn, cfg, 10)))
    # an int64 plane wraps modulo 2^64, as the device's sums do
    cfg = degree.config((0, 2), ("in_w",))
    big = np.iinfo(np.int64).max
    parts = [{"records": 1, "tombstones": 0, "out_total": 0, "in_total": 1, "out_skipped": 0, "in_skipped": 0,
              "first": 0, "count": 2, "in_w": np.array(v, dtype=np.int64)} for v in ([big, -5], [big, -6], [3, 11])]
    merged = degree.merge(parts)
    assert merged["in_w"].dtype == np.int64
    assert merged["in_w"].tolist() == [(2 * big + 3) - (1 << 64), 0] and merged["in_total"] == 3
    assert np.array_equal(degree.decode(degree.to_words(merged), cfg, 2)["in_w"], merged["in_w"])
    with pytest.raises(ValueError):
        degree.merge([])
    with pytest.raises(ValueError):
        degree.merge([parts[0], degree.reference(syn, degree.config((0, 3), ("in_w",)), 10)])
