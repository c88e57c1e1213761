"""CPU checks of the synapse select's boundary (abnn.h abnn_select_*): the
ctypes mirror matches the C layout, the constants and the TILE mirror,
abnn_select_words against select.n_words on valid and invalid configs, null
handles without a GPU, and the numpy restatement (abnn_amd.select.reference /
decode / to_words / merge) on a hand-made record array whose result is written
out by hand."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NONE = 0xFFFFFFFF
INF = float("inf")
NAN = float("nan")
SYN = [("src", "<u4"), ("dst", "<u4"), ("w", "<f4"), ("pad", "<f4")]


def test_select_config_layout_matches_c(tmp_path):
    from abnn_amd import _lib

    fields = [n for n, _ in _lib.SelectConfig._fields_]
    prog = tmp_path / "sz.c"
    prog.write_text('#include "abnn/abnn.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                    'int main(void){printf("%zu %d %u %u", sizeof(abnn_select_config), ABNN_SELECT_HEADER_WORDS,'
                    ' ABNN_SELECT_ANY, ABNN_SELECT_WEIGHT);\n'
                    + "".join(f'printf(" %zu", offsetof(abnn_select_config, {f}));\n' for f in fields)
                    + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(_lib.SelectConfig), _lib.SELECT_HEADER_WORDS, _lib.SELECT_ANY, _lib.SELECT_WEIGHT,
            *(getattr(_lib.SelectConfig, f).offset for f in fields)]
    assert got == want
    assert got[:4] == [32, 8, 1, 2]
    assert got[4:] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert fields == ["src_first", "src_count", "dst_first", "dst_count", "w_lo", "w_hi", "flags", "reserved"]


def test_tile_mirrors_the_header():
    from abnn_amd import select

    with open(os.path.join(ROOT, "abnn_amd", "csrc", "select.h")) as f:
        text = f.read()
    m = re.search(r"kSelectTile\s*=\s*(\d+)\s*;", text)
    assert m and int(m.group(1)) == select.TILE
    assert select.SYN_DTYPE == np.dtype(SYN)


def _invalid_configs():
    """name -> config: every refusal abnn.h lists that needs no handle (null is checked apart)."""
    from abnn_amd import select

    def edit(cfg, **kw):
        for k, v in kw.items():
            setattr(cfg, k, v)
        return cfg

    return {
        "flag bit 2": edit(select.config(dst=(0, 4)), flags=4),
        "flag bit 31 with valid bits": edit(select.config(dst=(0, 4), weights=(0.0, 1.0)), flags=2 | 1 << 31),
        "reserved": edit(select.config(dst=(0, 4)), reserved=1),
        "w_lo without WEIGHT": edit(select.config(dst=(0, 4)), w_lo=0.5),
        "w_hi without WEIGHT": edit(select.config(dst=(0, 4)), w_hi=1.0),
        "-0.0 without WEIGHT": edit(select.config(dst=(0, 4)), w_lo=-0.0),
        "w_lo NaN": select.config(weights=(NAN, 1.0)),
        "w_hi NaN": select.config(weights=(0.0, NAN)),
        "w_lo == w_hi": select.config(weights=(0.5, 0.5)),
        "w_lo > w_hi": select.config(weights=(0.5, 0.25)),
        "inf, inf": select.config(weights=(INF, INF)),
        "ANY with no range": select.config(any=True),
        "ANY with no range but weights": select.config(weights=(0.0, 1.0), any=True),
        "src wraps u32": select.config(src=(NONE, 2)),
        "dst wraps u32": select.config(dst=(2, NONE)),
    }


def _valid_configs():
    from abnn_amd import select

    return {
        "every record": select.config(),
        "dst": select.config(dst=(256, 256)),
        "src": select.config(src=(0, 256)),
        "both": select.config(src=(0, 1), dst=(999, 1)),
        "any": select.config(src=(512, 4096), dst=(512, 4096), any=True),
        "any, one range": select.config(dst=(5, 1), any=True),
        "weights": select.config(weights=(0.9, INF)),
        "weights from -inf": select.config(weights=(-INF, 0.0)),
        "everything at once": select.config(src=(1, 2), dst=(3, 4), weights=(-1.0, 1.0), any=True),
        "a range that ends at 2^32": select.config(src=(NONE, 1), dst=(0, NONE)),
        "first without a count": select.config(src=(77, 0)),
    }


def test_select_words():
    from abnn_amd import _lib, select

    lib = _lib.load()
    empty = np.zeros(0, dtype=SYN)
    for name, cfg in _valid_configs().items():
        for cap in (0, 1, 7, 65_536, 4_000_000_000, ((1 << 64) - 9) // 3):
            assert lib.abnn_select_words(C.byref(cfg), cap) == 8 + 3 * cap == select.n_words(cfg, cap), (name, cap)
        too_many = ((1 << 64) - 9) // 3 + 1  # 8 + 3 * capacity no longer fits 64 bits
        assert lib.abnn_select_words(C.byref(cfg), too_many) == 0 == select.n_words(cfg, too_many), name
    for name, cfg in _invalid_configs().items():
        for cap in (0, 5):
            assert lib.abnn_select_words(C.byref(cfg), cap) == 0, name
            assert select.n_words(cfg, cap) == 0, name
        with pytest.raises(ValueError):
            select.reference(empty, cfg, 4, 1000)
    assert lib.abnn_select_words(None, 4) == 0 and select.n_words(None, 4) == 0
    # the handle's check: a set range that ends above N_NRN (the reference takes n_nrn)
    for cfg in (select.config(src=(900, 101)), select.config(dst=(1000, 1)), select.config(src=(0, 1), dst=(0, 1001))):
        assert select.n_words(cfg, 4) == 20
        with pytest.raises(ValueError):
            select.reference(empty, cfg, 4, 1000)
    assert select.reference(empty, select.config(src=(900, 100)), 4, 1000)["matched"] == 0
    # config(): the flags follow the arguments
    assert select.config().flags == 0 and select.config(weights=(0.0, 1.0)).flags == _lib.SELECT_WEIGHT
    assert select.config(dst=(1, 2), any=True).flags == _lib.SELECT_ANY
    c = select.config(src=(1, 2), dst=(3, 4), weights=(0.25, 0.5), any=True)
    assert (c.src_first, c.src_count, c.dst_first, c.dst_count, c.w_lo, c.w_hi, c.flags, c.reserved) == \
        (1, 2, 3, 4, 0.25, 0.5, 3, 0)


def test_select_null_arguments_are_invalid_without_a_gpu():
    from abnn_amd import _lib, select

    lib = _lib.load()
    cfg = select.config(dst=(0, 4))
    out = (C.c_uint64 * 20)()
    assert lib.abnn_select_enqueue(None, C.byref(cfg), 4, out, None) == 1  # ABNN_ERR_INVALID
    assert lib.abnn_select(None, C.byref(cfg), 4, out, 20) == 1
    assert lib.abnn_select(None, None, 0, None, 0) == 1


W_LO, W_HI = 0.25, 0.75
DENORMAL = 1e-40


def _hand_made():
    """14 records over 10 neurons; the src range is 2..4, the dst range 3..5,
    the weight bounds [0.25, 0.75)."""
    rec = [
        (2, 3, 0.5),             # 0  both inside; weight inside
        (3, 3, NAN),             # 1  self-loop, both inside; NaN never passes a weight test
        (2, 9, W_LO),            # 2  src only; exactly w_lo: inside
        (8, 4, W_HI),            # 3  dst only; exactly w_hi: outside
        (NONE, NONE, 0.5),       # 4  tombstone
        (4, 4, INF),             # 5  self-loop, both inside; +inf: outside [0.25, 0.75), inside [0.25, +inf)
        (0, 1, 0.5),             # 6  neither; weight inside
        (3, 5, -INF),            # 7  both inside; -inf
        (9, 9, 0.5),             # 8  self-loop outside both ranges
        (4, 0, -0.0),            # 9  src only; -0.0
        (7, 5, DENORMAL),        # 10 dst only; a denormal
        (2, 2, 0.7499999),       # 11 self-loop: src inside (2..4), dst outside (3..5); just below w_hi
        (5, 3, 0.25000003),      # 12 dst only (src 5 is outside 2..4); just above w_lo
        (4, 5, 0.5),             # 13 both inside; weight inside
    ]
    syn = np.zeros(len(rec), dtype=SYN)
    for k, (s, d, w) in enumerate(rec):
        syn[k] = (s, d, F32(w), 0.0)
    return syn


SRC, DST = (2, 3), (3, 3)
# config arguments -> the indices that match, written out by hand
HAND_WANT = {
    "all": (dict(src=SRC, dst=DST), [0, 1, 5, 7, 13]),
    "any": (dict(src=SRC, dst=DST, any=True), [0, 1, 2, 3, 5, 7, 9, 10, 11, 12, 13]),
    "src only": (dict(src=SRC), [0, 1, 2, 5, 7, 9, 11, 13]),
    "dst only": (dict(dst=DST), [0, 1, 3, 5, 7, 10, 12, 13]),
    "src only, any": (dict(src=SRC, any=True), [0, 1, 2, 5, 7, 9, 11, 13]),
    "every live record": (dict(), [0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13]),
    "weights": (dict(weights=(W_LO, W_HI)), [0, 2, 6, 8, 11, 12, 13]),
    "all + weights": (dict(src=SRC, dst=DST, weights=(W_LO, W_HI)), [0, 13]),
    "any + weights": (dict(src=SRC, dst=DST, weights=(W_LO, W_HI), any=True), [0, 2, 11, 12, 13]),
    "at least w_lo": (dict(weights=(W_LO, INF)), [0, 2, 3, 6, 8, 11, 12, 13]),       # +inf itself is not below +inf
    "below w_lo": (dict(weights=(-INF, W_LO)), [7, 9, 10]),                          # -inf >= -inf
    "zero and the denormal": (dict(weights=(0.0, 1e-30)), [9, 10]),                  # -0.0 >= +0.0
    "negative": (dict(weights=(-INF, 0.0)), [7]),                                    # -0.0 < 0.0 is false
    "self-loops of 3 and 4": (dict(src=(3, 2), dst=(3, 2)), [1, 5]),
    "one neuron's neighbourhood": (dict(src=(5, 1), dst=(5, 1), any=True), [7, 10, 12, 13]),
}


@pytest.mark.parametrize("name", sorted(HAND_WANT))
def test_reference_known_answer(name):
    from abnn_amd import select

    syn = _hand_made()
    kw, want = HAND_WANT[name]
    cfg = select.config(**kw)
    offset = (1 << 32) + 5  # indices above 32 bits
    matched = len(want)
    for cap in sorted({0, 1, max(matched - 1, 0), matched, matched + 1}):
        got = select.reference(syn, cfg, cap, 10, syn_offset=offset)
        n = min(cap, matched)
        assert (got["records"], got["tombstones"], got["matched"], got["written"]) == (14, 1, matched, n), (name, cap)
        assert got["syn_offset"] == offset and got["capacity"] == cap
        assert got["index"].dtype == np.uint64 and got["syn"].dtype == np.dtype(SYN)
        assert got["index"].tolist() == [offset + i for i in want[:n]], (name, cap)
        assert np.array_equal(got["syn"].view(np.uint32), syn[want[:n]].view(np.uint32)), (name, cap)
        assert not got["syn"]["pad"].any()
        assert np.array_equal(select.matches(syn, cfg), np.isin(np.arange(14), want))


def test_reference_zeroes_the_pad_and_keeps_the_weight_bits():
    from abnn_amd import select

    syn = _hand_made()
    syn["pad"] = 3.0
    syn["w"][0] = np.array([0x7FC12345], dtype=np.uint32).view(F32)[0]  # a NaN with a payload
    got = select.reference(syn, select.config(src=(2, 1)), 5, 10)
    assert got["index"].tolist() == [0, 2, 11] and not got["syn"]["pad"].any()
    assert got["syn"]["w"].view(np.uint32)[0] == 0x7FC12345
    none = select.reference(syn[:0], select.config(), 3, 10, syn_offset=7)
    assert select.to_words(none).tolist() == [0, 0, 0, 0, 7, 0, 0, 0] + [0] * 9


def test_decode_and_to_words_round_trip():
    from abnn_amd import select

    syn = _hand_made()
    for name, (kw, want) in HAND_WANT.items():
        cfg = select.config(**kw)
        for cap in (0, 1, len(want), len(want) + 3):
            d = select.reference(syn, cfg, cap, 10, syn_offset=(1 << 40))
            words = select.to_words(d)
            assert words.dtype == np.uint64 and words.shape == (select.n_words(cfg, cap),)
            assert not words[5:8].any()
            back = select.decode(words, cap)
            assert set(back) == set(d)
            assert np.array_equal(select.to_words(back), words)
            for k, v in d.items():
                assert np.array_equal(np.asarray(back[k]).view(np.uint8) if k == "syn" else back[k],
                                      np.asarray(v).view(np.uint8) if k == "syn" else v), (name, k)
    # the layout: header, the index plane of `capacity` words, the record plane of 2 * capacity
    d = select.reference(syn, select.config(src=SRC, dst=DST), 7, 10, syn_offset=100)
    words = select.to_words(d)
    assert words[:8].tolist() == [14, 1, 5, 5, 100, 0, 0, 0]
    assert words[8:15].tolist() == [100, 101, 105, 107, 113, 0, 0]
    rec = words[15:].view(np.uint32).reshape(7, 4)
    assert rec[:, 0].tolist() == [2, 3, 4, 3, 4, 0, 0] and rec[:, 1].tolist() == [3, 3, 4, 5, 5, 0, 0]
    assert rec[:, 2].tolist() == syn["w"][[0, 1, 5, 7, 13]].view(np.uint32).tolist() + [0, 0] and not rec[:, 3].any()


def test_merge_of_a_three_way_split():
    from abnn_amd import select

    syn = _hand_made()
    cuts = ((0, 5), (5, 9), (9, 14))
    for name, (kw, want) in HAND_WANT.items():
        cfg = select.config(**kw)
        for cap in sorted({0, 1, 2, max(len(want) - 1, 0), len(want), len(want) + 2}):
            whole = select.reference(syn, cfg, cap, 10, syn_offset=1 << 33)
            parts = [select.reference(syn[a:b], cfg, cap, 10, syn_offset=(1 << 33) + a) for a, b in cuts]
            assert [p["records"] for p in parts] == [5, 4, 5]
            merged = select.merge(parts, cap)
            assert np.array_equal(select.to_words(merged), select.to_words(whole)), (name, cap)
            assert merged["written"] == min(cap, len(want)) and merged["matched"] == len(want)
            # parts that hold only what the merged result takes from them
            need, lean = cap, []
            for (a, b) in cuts:
                p = select.reference(syn[a:b], cfg, need, 10, syn_offset=(1 << 33) + a)
                need -= p["written"]
                lean.append(p)
            assert np.array_equal(select.to_words(select.merge(lean, cap)), select.to_words(whole)), (name, cap)
    with pytest.raises(ValueError):
        select.merge([], 4)
    cfg = select.config()
    short = [select.reference(syn[a:b], cfg, 1, 10, syn_offset=a) for a, b in cuts]
    with pytest.raises(ValueError):
        select.merge(short, 6)  # the first part was cut below what the merged result needs
