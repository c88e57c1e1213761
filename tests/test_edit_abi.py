"""CPU checks of the synapse edit's boundary (abnn.h abnn_edit_*): the ctypes
mirror matches the C layout, abnn_edit_words against edit.n_words on valid
configs and on every refusal, null arguments without a GPU, abnn_edit_host and
abnn_edit_factors_host against the numpy restatement (abnn_amd.edit) bit for
bit, a hand-made record array whose results are written out by hand, a DRAW
spread over shards, the scaling bound on the reference alone, and the host rule
in a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NONE = 0xFFFFFFFF
INF = float("inf")
SYN = [("src", "<u4"), ("dst", "<u4"), ("w", "<f4"), ("pad", "<f4")]
SPECIAL = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-40, 0.25, 0.75, 0.7499999, 0.25000003], dtype=F32)
SMALL_CONFIGS = (dict(), dict(dst=(256, 256)), dict(src=(0, 500)), dict(src=(100, 600), dst=(300, 600)),
                 dict(src=(0, 100), dst=(900, 100), any=True), dict(dst=(999, 1), any=True),
                 dict(weights=(0.25, 0.75)), dict(src=(0, 500), weights=(0.25, INF)),
                 dict(src=(0, 300), dst=(0, 300), weights=(-INF, 0.25), any=True))
OPS = {"set": dict(b=0.625), "affine": dict(a=-1.5, b=0.125), "scale_dst": dict(), "scale_src": dict(),
       "draw": dict(a=-0.25, b=0.5, seed=0xC0FFEE), "kill": dict()}
N_NRN = 1000


def test_edit_config_layout_matches_c(tmp_path):
    from abnn_amd import _lib

    fields = [n for n, _ in _lib.EditConfig._fields_]
    consts = ["ABNN_EDIT_HEADER_WORDS", "ABNN_EDIT_ANY", "ABNN_EDIT_WEIGHT", "ABNN_EDIT_CLAMP", "ABNN_SELECT_ANY",
              "ABNN_SELECT_WEIGHT", "ABNN_EDIT_SET", "ABNN_EDIT_AFFINE", "ABNN_EDIT_SCALE_DST", "ABNN_EDIT_SCALE_SRC",
              "ABNN_EDIT_DRAW", "ABNN_EDIT_KILL"]
    prog = tmp_path / "sz.c"
    prog.write_text('#include "abnn/abnn.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                    'int main(void){printf("%zu %llu", sizeof(abnn_edit_config), (unsigned long long)ABNN_EDIT_KEY);\n'
                    + "".join(f'printf(" %u", (unsigned)({c}));\n' for c in consts)
                    + "".join(f'printf(" %zu", offsetof(abnn_edit_config, {f}));\n' for f in fields)
                    + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(_lib.EditConfig), _lib.EDIT_KEY, _lib.EDIT_HEADER_WORDS, _lib.EDIT_ANY, _lib.EDIT_WEIGHT,
            _lib.EDIT_CLAMP, _lib.SELECT_ANY, _lib.SELECT_WEIGHT, _lib.EDIT_SET, _lib.EDIT_AFFINE, _lib.EDIT_SCALE_DST,
            _lib.EDIT_SCALE_SRC, _lib.EDIT_DRAW, _lib.EDIT_KILL, *(getattr(_lib.EditConfig, f).offset for f in fields)]
    assert got == want
    assert got[0] == 64 and got[2:14] == [8, 1, 2, 4, 1, 2, 0, 1, 2, 3, 4, 5]
    assert got[14:] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 56]
    assert fields == ["src_first", "src_count", "dst_first", "dst_count", "w_lo", "w_hi", "flags", "op", "a", "b",
                      "c_lo", "c_hi", "seed", "reserved"]
    assert _lib.EDIT_KEY != _lib.GRAPH_KEY


def _valid_configs():
    from abnn_amd import edit

    out = []
    for op, params in OPS.items():
        for kw in SMALL_CONFIGS:
            if op.startswith("scale") and kw.get("any"):
                continue
            out.append(edit.config(op, **params, **kw))
            if op != "kill":
                out.append(edit.config(op, clamp=(0.0, 0.5), **params, **kw))
    out += [edit.config("set", b=INF), edit.config("affine", a=-INF, b=INF), edit.config("draw", a=0.5, b=0.5),
            edit.config("set", b=-0.0, clamp=(-INF, INF)), edit.config("set", clamp=(0.25, 0.25)),
            edit.config("draw", a=0.0, b=0.0, seed=2**64 - 1), edit.config("kill", weights=(-INF, INF))]
    return out


def _invalid_configs():
    """name -> config: every refusal abnn.h lists (null is checked apart)."""
    from abnn_amd import edit

    def tweak(cfg, **fields):
        for k, v in fields.items():
            setattr(cfg, k, v)
        return cfg

    bad = {
        # the shared fields: what abnn_select_words refuses
        "src range wraps u32": edit.config("set", src=(0xFFFFFFFF, 2)),
        "dst range wraps u32": edit.config("kill", dst=(2, 0xFFFFFFFF)),
        "ANY with neither range": edit.config("set", any=True),
        "w_lo without WEIGHT": tweak(edit.config("set"), w_lo=0.5),
        "-0.0 w_hi without WEIGHT": tweak(edit.config("set"), w_hi=-0.0),
        "NaN w_lo": edit.config("set", weights=(np.nan, 1.0)),
        "NaN w_hi": edit.config("set", weights=(0.0, np.nan)),
        "w_lo == w_hi": edit.config("set", weights=(0.5, 0.5)),
        "w_lo > w_hi": edit.config("set", weights=(0.5, 0.25)),
        # the edit's own
        "unknown op": tweak(edit.config("set"), op=6),
        "unknown flag bit 8": tweak(edit.config("set"), flags=8),
        "unknown flag bit 31": tweak(edit.config("set"), flags=1 << 31),
        "reserved[0]": edit.config("set"),
        "reserved[1]": edit.config("set"),
        "a set for SET": edit.config("set", a=1.0, b=1.0),
        "a -0.0 for KILL": edit.config("kill", a=-0.0),
        "b set for KILL": edit.config("kill", b=0.5),
        "a set for SCALE_DST": edit.config("scale_dst", a=2.0),
        "b set for SCALE_SRC": edit.config("scale_src", b=2.0),
        "c_lo without CLAMP": tweak(edit.config("set"), c_lo=0.5),
        "c_hi without CLAMP": tweak(edit.config("affine", a=1.0), c_hi=0.5),
        "seed for SET": edit.config("set", seed=1),
        "seed for KILL": edit.config("kill", seed=1 << 63),
        "NaN b for SET": edit.config("set", b=np.nan),
        "NaN a for AFFINE": edit.config("affine", a=np.nan, b=1.0),
        "NaN b for AFFINE": edit.config("affine", a=1.0, b=np.nan),
        "NaN a for DRAW": edit.config("draw", a=np.nan, b=1.0),
        "NaN c_lo": edit.config("set", clamp=(np.nan, 1.0)),
        "NaN c_hi": edit.config("set", clamp=(0.0, np.nan)),
        "c_lo > c_hi": edit.config("set", clamp=(0.5, 0.25)),
        "DRAW a > b": edit.config("draw", a=0.5, b=0.25),
        "DRAW a -inf": edit.config("draw", a=-INF, b=0.25),
        "DRAW b inf": edit.config("draw", a=0.0, b=INF),
        "CLAMP with KILL": edit.config("kill", clamp=(0.0, 1.0)),
        "ANY with SCALE_DST": edit.config("scale_dst", dst=(0, 10), any=True),
        "ANY with SCALE_SRC": edit.config("scale_src", src=(0, 10), dst=(5, 5), any=True),
    }
    bad["reserved[0]"].reserved[0] = 1
    bad["reserved[1]"].reserved[1] = 1
    return bad


def test_edit_words():
    from abnn_amd import _lib, edit

    lib = _lib.load()
    valid = _valid_configs()
    assert len(valid) > 90
    for cfg in valid:
        assert lib.abnn_edit_words(C.byref(cfg)) == 8 == edit.n_words(cfg), bytes(cfg).hex()
    empty = np.zeros(0, dtype=SYN)
    for name, cfg in _invalid_configs().items():
        assert lib.abnn_edit_words(C.byref(cfg)) == 0, name
        assert edit.n_words(cfg) == 0, name
        with pytest.raises(ValueError):
            edit.reference(empty, cfg, N_NRN, plane=np.ones(N_NRN, F32) if cfg.op in (2, 3) else None)
        out = (C.c_uint64 * 8)()
        assert lib.abnn_edit_host(C.byref(cfg), N_NRN, 0, None, 0, None, out) == 1, name
    assert lib.abnn_edit_words(None) == 0
    cfg = edit.config("affine", src=(1, 2), dst=(3, 4), weights=(0.25, 0.5), any=True, a=2.0, b=3.0, clamp=(0.5, 4.0))
    assert (cfg.src_first, cfg.src_count, cfg.dst_first, cfg.dst_count, cfg.w_lo, cfg.w_hi, cfg.flags, cfg.op, cfg.a,
            cfg.b, cfg.c_lo, cfg.c_hi, cfg.seed) == (1, 2, 3, 4, 0.25, 0.5, 7, 1, 2.0, 3.0, 0.5, 4.0, 0)
    assert edit.config(5).op == edit.config("kill").op == 5 and edit.config("draw", seed=-1).seed == 2**64 - 1
    assert edit.merge([edit.decode(np.arange(8, dtype=np.uint64)), edit.decode(np.arange(8, dtype=np.uint64))]) == dict(
        zip(edit.KEYS, (0, 2, 4, 6, 8, 10)))


def test_null_and_range_arguments_are_invalid_without_a_gpu():
    from abnn_amd import _lib, edit

    lib = _lib.load()
    cfg, scale = edit.config("set", b=1.0), edit.config("scale_dst", dst=(0, 4))
    out = (C.c_uint64 * 8)()
    rec = np.zeros(4, dtype=SYN)
    plane = np.ones(4, dtype=F32)
    assert lib.abnn_edit_enqueue(None, C.byref(cfg), None, out, None) == 1  # ABNN_ERR_INVALID
    assert lib.abnn_edit(None, C.byref(cfg), None, 0, out) == 1
    assert lib.abnn_edit(None, None, None, 0, None) == 1
    assert lib.abnn_edit_factors_enqueue(None, None, 0, 1.0, 0.5, 2.0, None, None) == 1
    assert lib.abnn_edit_host(None, N_NRN, 0, rec.ctypes.data, 4, None, out) == 1
    assert lib.abnn_edit_host(C.byref(cfg), N_NRN, 0, None, 4, None, out) == 1
    assert lib.abnn_edit_host(C.byref(cfg), N_NRN, 0, rec.ctypes.data, 4, None, None) == 1
    assert lib.abnn_edit_host(C.byref(cfg), N_NRN, 0, rec.ctypes.data, 4, plane.ctypes.data, out) == 1  # superfluous
    assert lib.abnn_edit_host(C.byref(scale), N_NRN, 0, rec.ctypes.data, 4, None, out) == 1  # missing
    assert lib.abnn_edit_host(C.byref(edit.config("set", dst=(990, 11))), N_NRN, 0, rec.ctypes.data, 4, None, out) == 1
    assert lib.abnn_edit_host(C.byref(edit.config("set", src=(1000, 1))), N_NRN, 0, rec.ctypes.data, 4, None, out) == 1
    assert lib.abnn_edit_host(C.byref(scale), N_NRN, 0, rec.ctypes.data, 4, plane.ctypes.data, out) == 0
    assert lib.abnn_edit_host(C.byref(cfg), N_NRN, 0, None, 0, None, out) == 0 and not any(out)
    words = np.ones(4, dtype=np.int64)
    for target, lo, hi in ((0.0, 0.5, 2.0), (-1.0, 0.5, 2.0), (INF, 0.5, 2.0), (np.nan, 0.5, 2.0), (1.0, 0.0, 2.0),
                           (1.0, 2.0, 0.5), (1.0, 0.5, INF), (1.0, np.nan, 2.0), (1.0, 0.5, np.nan)):
        assert lib.abnn_edit_factors_host(words.ctypes.data, 4, target, lo, hi, plane.ctypes.data) == 1, (target, lo, hi)
        with pytest.raises(ValueError):
            edit.factors(words, target, lo, hi)
    assert lib.abnn_edit_factors_host(None, 4, 1.0, 0.5, 2.0, plane.ctypes.data) == 1
    assert lib.abnn_edit_factors_host(words.ctypes.data, 4, 1.0, 0.5, 2.0, plane.ctypes.data) == 0


def _records(n, seed):
    """The select tests' records with tombstones: uniform src / dst over 1000
    neurons, weights in [-0.1, 1.1], the special values at the first, a middle
    and the last index."""
    rng = np.random.default_rng(seed)
    syn = np.zeros(n, dtype=SYN)
    syn["src"] = rng.integers(0, N_NRN, n, dtype=np.uint32)
    syn["dst"] = rng.integers(0, N_NRN, n, dtype=np.uint32)
    syn["w"] = rng.uniform(-0.1, 1.1, n).astype(F32)
    k = len(SPECIAL)
    if n >= 3 * k:
        for at in (0, n // 2 - k // 2, n - k):
            syn["w"][at:at + k] = SPECIAL
        syn["src"][5::13] = syn["dst"][5::13] = NONE
    elif n:
        for j, at in enumerate(sorted({0, n // 2, n - 1})):
            syn["w"][at] = SPECIAL[(seed + j) % k]
    return syn


def _host(cfg, syn, syn_offset=0, plane=None, n_nrn=N_NRN):
    from abnn_amd import _lib, edit

    got = np.ascontiguousarray(syn).copy()
    out = np.zeros(8, dtype=np.uint64)
    st = _lib.load().abnn_edit_host(C.byref(cfg), n_nrn, syn_offset, got.ctypes.data, len(got),
                                    None if plane is None else plane.ctypes.data, out.ctypes.data)
    assert st == 0, _lib.load().abnn_last_error()
    assert out[6] == 0 and out[7] == 0
    return got, edit.decode(out)


def _cases():
    """(config, plane) over every op, with and without CLAMP, over the select
    tests' range / weight combinations."""
    from abnn_amd import edit

    rng = np.random.default_rng(2)
    for op, params in OPS.items():
        for kw in SMALL_CONFIGS:
            if op.startswith("scale") and kw.get("any"):
                continue
            for clamp in (None, (0.0, 0.5)):
                if op == "kill" and clamp:
                    continue
                cfg = edit.config(op, clamp=clamp, **params, **kw)
                plane = None
                if op.startswith("scale"):
                    plane = rng.uniform(0.25, 1.75, edit.plane_range(cfg, N_NRN)[1]).astype(F32)
                    plane[::11], plane[3::11], plane[5::11], plane[7::11] = 0.0, 1.0, np.nan, 3.4e38
                yield cfg, plane


@pytest.mark.parametrize("n", [0, 1, 2, 3, 65, 10_000])
def test_host_rule_equals_the_numpy_restatement(n):
    from abnn_amd import edit

    syn = _records(n, 3)
    seen = 0
    for cfg, plane in _cases():
        offset = 5_000_000_123 if cfg.op == edit.OPS["draw"] else 0
        want, head = edit.reference(syn, cfg, N_NRN, offset, plane)
        got, ghead = _host(cfg, syn, offset, plane)
        assert got.tobytes() == want.tobytes(), (n, bytes(cfg).hex())
        assert ghead == head and head["records"] == n
        seen += head["changed"]
    assert seen > 0 or n == 0
    if n == 10_000:  # the cases reach what they are for
        want, head = edit.reference(syn, edit.config("scale_dst"), N_NRN, 0, np.where(np.arange(N_NRN) % 2, np.nan, 3e38).astype(F32))
        assert head["nonfinite"] > 4000 and head["tombstones"] == len(syn[5::13])
        assert edit.reference(syn, edit.config("affine", a=1.0, b=0.0), N_NRN)[1]["changed"] < 30  # -0.0, payloads


def test_hand_made_records():
    """Ten records over ten neurons; the expected results are written out by hand."""
    from abnn_amd import edit

    nan = np.nan
    rec = np.array([(0, 5, 0.5, 0), (1, 5, 0.25, 0), (2, 6, -0.0, 0), (NONE, NONE, 0.75, 0), (3, 7, 1.0, 0),
                    (4, 7, nan, 0), (0, 8, INF, 0), (9, 9, 0.125, 0), (5, 5, 2.0, 0), (1, 6, 0.375, 0)], dtype=SYN)

    def run(cfg, plane=None):
        got, head = _host(cfg, rec, 0, plane, n_nrn=10)
        want, whead = edit.reference(rec, cfg, 10, 0, plane)
        assert got.tobytes() == want.tobytes() and head == whead
        return got, [head[k] for k in edit.KEYS]

    # SET 0.5 on dst 5..6: records 0, 1, 2, 8, 9 match; record 0 already holds 0.5
    got, head = run(edit.config("set", b=0.5, dst=(5, 2)))
    assert got["w"].tolist()[:3] == [0.5, 0.5, 0.5] and got["w"][8] == 0.5 and got["w"][9] == 0.5
    assert got["w"][4] == 1.0 and got["w"][3] == 0.75 and head == [10, 1, 5, 4, 0, 0]
    # AFFINE w * 2 + 0.25, clamped to [0, 1.5], on weights in [0.25, 1.5): records 0, 1, 4, 9 (not the tombstone's 0.75)
    got, head = run(edit.config("affine", a=2.0, b=0.25, weights=(0.25, 1.5), clamp=(0.0, 1.5)))
    assert [got["w"][i] for i in (0, 1, 4, 9)] == [1.25, 0.75, 1.5, 1.0]
    assert got["w"][3] == 0.75 and got["w"][8] == 2.0 and np.isnan(got["w"][5]) and head == [10, 1, 4, 4, 0, 0]
    # KILL src 0..1 or dst 9: records 0, 1, 6, 7, 9
    got, head = run(edit.config("kill", src=(0, 2), dst=(9, 1), any=True))
    assert got["src"].tolist() == [NONE, NONE, 2, NONE, 3, 4, NONE, NONE, 5, NONE]
    assert got["dst"].tolist() == [NONE, NONE, 6, NONE, 7, 7, NONE, NONE, 5, NONE]
    assert got["w"].view(np.uint32).tolist() == rec["w"].view(np.uint32).tolist() and head == [10, 1, 5, 5, 5, 0]
    # SCALE_DST over dst 5..8 with factors 2, 1, 0.5, 0: inf * 0 is the canonical NaN, -0.0 * 1 is unchanged
    got, head = run(edit.config("scale_dst", dst=(5, 4)), np.array([2.0, 1.0, 0.5, 0.0], dtype=F32))
    assert [got["w"][i] for i in (0, 1, 2, 4, 8, 9)] == [1.0, 0.5, -0.0, 0.5, 4.0, 0.375]
    assert got["w"].view(np.uint32)[[5, 6]].tolist() == [0x7FC00000, 0x7FC00000] and got["w"][7] == 0.125
    assert np.signbit(got["w"][2]) and head == [10, 1, 8, 5, 0, 2]


def test_factors_host_equals_the_numpy_restatement():
    from abnn_amd import _lib, edit

    lib = _lib.load()
    rng = np.random.default_rng(6)
    words = np.concatenate([
        np.array([0, -1, -(1 << 40), 1, 1 << 24, (1 << 53) + 1, (1 << 53) + 3, (1 << 60) + (1 << 36), (1 << 62) + 12345,
                  (1 << 24) + 1, (1 << 25) + 1, (1 << 25) + 3, 3 << 22, 1 << 20, 1 << 30, -(1 << 63)], dtype=np.int64),
        rng.integers(-(1 << 30), 1 << 34, 5000), rng.integers(0, 1 << 62, 5000)])
    for target, lo, hi in ((1.0, 0.5, 2.0), (153.6, 0.5, 2.0), (100.0, 1e-30, 1e30), (3e-5, 1e-38, 3e38), (1.0, 1.0, 1.0)):
        got = np.zeros(len(words), dtype=F32)
        assert lib.abnn_edit_factors_host(words.ctypes.data, len(words), target, lo, hi, got.ctypes.data) == 0
        want = edit.factors(words, target, lo, hi)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (target, lo, hi)
        assert (want >= F32(lo)).all() and (want <= F32(hi)).all()
    f = edit.factors(words[:16], 1.0, 0.5, 2.0)
    assert f.tolist() == [1.0, 1.0, 1.0, 2.0, 1.0, 0.5, 0.5, 0.5, 0.5, 1.0, 0.5, 0.5, 1.3333333730697632, 2.0, 0.5, 1.0]
    # above 2**53 the conversion rounds: (1 << 53) + 1 and + 3 convert like their float32 neighbours
    assert F32(np.int64((1 << 25) + 1)) == F32(1 << 25) and F32(np.int64((1 << 25) + 3)) == F32((1 << 25) + 4)
    assert edit.factors(np.array([(1 << 25) + 3], dtype=np.int64), 2.0, 1e-9, 1e9)[0] == F32(2.0) / (
        F32((1 << 25) + 4) * F32(2.0**-24))


def test_draw_spreads_over_shards():
    from abnn_amd import edit

    n = 10_000
    syn = _records(n, 8)
    for kw in (dict(), dict(src=(0, 700)), dict(weights=(0.0, 0.5))):
        cfg = edit.config("draw", a=-0.25, b=0.75, seed=0xFEED, **kw)
        whole, head = edit.reference(syn, cfg, N_NRN, 77)
        for k in (1, 3_333, 4_096, n - 1):
            lo, h0 = edit.reference(syn[:k], cfg, N_NRN, 77)
            hi, h1 = edit.reference(syn[k:], cfg, N_NRN, 77 + k)
            assert np.concatenate([lo, hi]).tobytes() == whole.tobytes(), k
            assert edit.merge([h0, h1]) == head
            got, _ = _host(cfg, syn[k:], 77 + k)
            assert got.tobytes() == hi.tobytes()
        from abnn_amd import select

        drawn = whole["w"][select.matches(syn, select.config(**kw))]
        assert len(drawn) > 3000 and (drawn >= F32(-0.25)).all() and (drawn <= F32(0.75)).all()
        assert len(np.unique(drawn)) > 0.99 * len(drawn)
    other, _ = edit.reference(syn, edit.config("draw", a=-0.25, b=0.75, seed=0xFEED + 1), N_NRN, 77)
    assert not np.array_equal(other["w"], edit.reference(syn, edit.config("draw", a=-0.25, b=0.75, seed=0xFEED), N_NRN, 77)[0]["w"])


def test_scaling_bound_on_the_reference():
    """The bound test_edit_gpu.py relies on, on the CPU alone: the generated
    small graph scaled by edit.reference stays inside it, and at most 1 % of the
    outputs are left out."""
    from abnn_amd import degree, edit, graph

    from test_edit_gpu import _scaling_graph, scaling_bound_holds

    before = graph.reference(_scaling_graph())
    assert len(before) == 100_000
    for target in (100.0, 153.6, 200.0):
        in_w = degree.reference(before, degree.config((256, 256), ("in_w",)), N_NRN)["in_w"]
        f = edit.factors(in_w, target, 0.5, 2.0)
        after, head = edit.reference(before, edit.config("scale_dst", dst=(256, 256)), N_NRN, plane=f)
        assert head["matched"] == 65_536 and head["nonfinite"] == 0
        assert scaling_bound_holds(before, after, f, target, (0.5, 2.0), N_NRN) <= 2


def test_host_rule_under_the_sanitizers(tmp_path):
    """csrc/edit.h's host rule in a stand-alone program built with
    -fsanitize=address,undefined, run once over small arrays of every op."""
    from abnn_amd import edit
    from abnn_amd.build import build_edit_host_test

    prog = build_edit_host_test(out=str(tmp_path / "edit_host_test"))
    cases = []
    for n in (0, 1, 3, 65, 1000):
        syn = _records(n, n + 1)
        cases += [(cfg, plane, syn, 123 if cfg.op == 4 else 0) for cfg, plane in _cases()]
    words = np.array([0, -7, 1, 1 << 24, (1 << 53) + 1, 3 << 22, -(1 << 63), (1 << 62) + 5], dtype=np.int64)
    blob = [struct.pack("<Q", len(cases))]
    for cfg, plane, syn, offset in cases:
        m = 0 if plane is None else len(plane)
        blob += [bytes(cfg), struct.pack("<4Q", N_NRN, offset, len(syn), m), syn.tobytes(), b"" if plane is None else plane.tobytes()]
    blob += [struct.pack("<Q4f", len(words), 1.0, 0.5, 2.0, 0.0), words.tobytes()]
    (tmp_path / "in.bin").write_bytes(b"".join(blob))
    r = subprocess.run([prog, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    out = (tmp_path / "out.bin").read_bytes()
    at = 0
    for cfg, plane, syn, offset in cases:
        want, head = edit.reference(syn, cfg, N_NRN, offset, plane)
        got_head = np.frombuffer(out, dtype=np.uint64, count=8, offset=at)
        at += 64
        assert edit.decode(got_head) == head
        assert out[at:at + 16 * len(syn)] == want.tobytes(), bytes(cfg).hex()
        at += 16 * len(syn)
    got = np.frombuffer(out, dtype=np.uint32, count=len(words), offset=at)
    assert got.tolist() == edit.factors(words, 1.0, 0.5, 2.0).view(np.uint32).tolist() and at + 4 * len(words) == len(out)
