"""CPU checks of the graph builder's boundary (abnn.h abnn_graph_*): the ctypes
mirrors match the C layout and constants, abnn_graph_records against
graph.records on valid specs and on every refusal abnn.h lists, the host rule
(abnn_graph_fill_host) against its numpy restatement (graph.reference) bit for
bit, a hand-written six-record expectation, the ring lattice's degrees, the
Beta law's mean, and null arguments without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
INF = float("inf")
NAN = float("nan")


def test_graph_struct_layouts_match_c(tmp_path):
    from abnn_amd import _lib

    bf = [n for n, _ in _lib.GraphBlock._fields_]
    sf = [n for n, _ in _lib.GraphSpec._fields_]
    prog = tmp_path / "sz.c"
    prog.write_text('#include "abnn/abnn.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                    'int main(void){printf("%zu %zu %d %llu %u %u %u %u %u", sizeof(abnn_graph_block),'
                    ' sizeof(abnn_graph_spec), ABNN_GRAPH_MAX_BLOCKS, (unsigned long long)ABNN_GRAPH_KEY,'
                    ' ABNN_TOPO_DENSE, ABNN_TOPO_RANDOM, ABNN_TOPO_RING, ABNN_W_UNIFORM, ABNN_W_BETA);\n'
                    + "".join(f'printf(" %zu", offsetof(abnn_graph_block, {f}));\n' for f in bf)
                    + "".join(f'printf(" %zu", offsetof(abnn_graph_spec, {f}));\n' for f in sf)
                    + 'printf(" %d\\n", ABNN_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(_lib.GraphBlock), C.sizeof(_lib.GraphSpec), _lib.GRAPH_MAX_BLOCKS, _lib.GRAPH_KEY,
            _lib.TOPO_DENSE, _lib.TOPO_RANDOM, _lib.TOPO_RING, _lib.W_UNIFORM, _lib.W_BETA,
            *(getattr(_lib.GraphBlock, f).offset for f in bf), *(getattr(_lib.GraphSpec, f).offset for f in sf), 10]
    assert got == want
    assert got[:9] == [64, 1040, 16, 0xD1B54A32D192ED03, 0, 1, 2, 0, 1]
    assert bf == ["count", "src_first", "src_count", "dst_first", "dst_count", "topology", "k", "p_rewire",
                  "weight_law", "w_lo", "w_hi", "beta_a", "beta_b", "reserved"]
    assert got[9:9 + len(bf)] == [0, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52, 56]
    assert sf == ["seed", "n_blocks", "reserved", "blocks"] and got[9 + len(bf):-1] == [0, 8, 12, 16]


def _mixed_spec(seed=0xFEEDFACE12345678):
    """All three topologies and both laws; the block boundaries fall at 129,
    130, 40 131, 70 131, 70 136, 71 151: 1, 2, 3, 3, 0, 3 mod 4."""
    from abnn_amd import graph

    return graph.spec([
        graph.dense((0, 16), (16, 8), graph.uniform(0.4, 0.8), count=129),        # S * D = 128: wraps by one
        graph.random((24, 100), (30, 7), 1, graph.beta(2, 8)),                     # a one-record block
        graph.random((24, 4072), (24, 4072), 40_001, graph.uniform(0.1, 0.2)),
        graph.small_world((100, 3000), 10, 0.1, graph.beta(2, 8, 0.0, 0.5), count=30_000),
        graph.small_world((100, 9), 8, 0.0, graph.beta(9, 3, -1.0, 1.0), count=5),  # a 5-record block, keeps the largest
        graph.small_world((7, 203), 5, 1.0, graph.uniform(0.25, 0.25)),           # 1015 records, all rewired; w_lo == w_hi
    ], seed)


def _valid_specs():
    from abnn_amd import graph

    u = graph.uniform(0.0, 1.0)
    big = (1 << 59) - 1
    return {
        "mixed": _mixed_spec(),
        "one dense block": graph.spec([graph.dense((0, 2), (2, 2), u)], 1),
        "sixteen blocks of the largest count": graph.spec([graph.random((0, 5), (5, 5), big, u)] * 16, 0),
        "populations that end at 2^32": graph.spec([graph.random((0xFFFFFFFF, 1), (1, 0xFFFFFFFF), 3, u)], 2),
        "ring with k = n - 1": graph.spec([graph.small_world((3, 6), 5, 0.5, u)], 3),
        "ring with p = 1": graph.spec([graph.small_world((0, 2), 1, 1.0, graph.beta(1, 1))], 4),
        "beta(8, 8): fifteen draws": graph.spec([graph.random((0, 9), (0, 9), 7, graph.beta(8, 8))], 5),
        "beta(15, 1) and beta(1, 15)": graph.spec([graph.random((0, 9), (0, 9), 7, graph.beta(15, 1)),
                                                   graph.random((0, 9), (0, 9), 7, graph.beta(1, 15))], 6),
        "negative bounds": graph.spec([graph.dense((0, 1), (0, 1), graph.uniform(-2.0, -1.0))], (1 << 64) - 1),
    }


def _invalid_specs():
    """name -> spec: every refusal abnn.h lists, one case each (null is checked apart)."""
    from abnn_amd import _lib, graph

    u = graph.uniform(0.0, 1.0)

    def one(block=None, **kw):
        s = graph.spec([graph.random((0, 10), (10, 10), 100, u) if block is None else block], 1)
        for k, v in kw.items():
            setattr(s.blocks[0], k, v)
        return s

    def spec_edit(**kw):
        s = one()
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    ring = graph.small_world((5, 10), 4, 0.5, u)
    past = one()
    past.blocks[1].w_hi = 1.0
    res_block = one()
    res_block.blocks[0].reserved[1] = 1
    return {
        "n_blocks 0": spec_edit(n_blocks=0),
        "n_blocks 17": spec_edit(n_blocks=17),
        "spec reserved": spec_edit(reserved=1),
        "block reserved": res_block,
        "a non-zero block past n_blocks": past,
        "count 0": one(count=0),
        "count 2^59": one(count=1 << 59),
        "S == 0": one(src_count=0),
        "D == 0": one(dst_count=0),
        "src wraps u32": one(src_first=0xFFFFFFFF, src_count=2),
        "dst wraps u32": one(dst_first=2, dst_count=0xFFFFFFFF),
        "unknown topology": one(topology=3),
        "unknown weight law": one(weight_law=2),
        "k on a RANDOM block": one(k=1),
        "p_rewire on a DENSE block": one(graph.dense((0, 2), (2, 2), u), p_rewire=0.5),
        "-0.0 p_rewire on a RANDOM block": one(p_rewire=-0.0),
        "RING with different firsts": one(ring, dst_first=6),
        "RING with different counts": one(ring, dst_count=11),
        "RING k == 0": one(ring, k=0),
        "RING k == n": one(ring, k=10),
        "RING p < 0": one(ring, p_rewire=-0.25),
        "RING p > 1": one(ring, p_rewire=1.5),
        "RING p NaN": one(ring, p_rewire=NAN),
        "beta_a on a UNIFORM block": one(beta_a=1),
        "beta_b on a UNIFORM block": one(beta_b=1),
        "BETA a == 0": one(graph.random((0, 10), (10, 10), 100, graph.beta(0, 3))),
        "BETA b == 0": one(graph.random((0, 10), (10, 10), 100, graph.beta(3, 0))),
        "BETA a + b - 1 == 16": one(graph.random((0, 10), (10, 10), 100, graph.beta(8, 9))),
        "w_lo -inf": one(w_lo=-INF),
        "w_hi inf": one(w_hi=INF),
        "w_lo NaN": one(w_lo=NAN),
        "w_hi NaN": one(w_hi=NAN),
        "w_lo > w_hi": one(w_lo=0.5, w_hi=0.25),
        "the second block invalid": graph.spec([graph.random((0, 10), (10, 10), 100, u),
                                                _lib.GraphBlock(0, 0, 10, 10, 10, 1, 0, 0.0, 0, 0.0, 1.0, 0, 0)], 1),
    }


def test_graph_records():
    from abnn_amd import _lib, graph

    lib = _lib.load()
    for name, s in _valid_specs().items():
        want = sum(int(s.blocks[j].count) for j in range(s.n_blocks))
        assert lib.abnn_graph_records(C.byref(s)) == want == graph.records(s) != 0, name
    assert graph.records(_mixed_spec()) == 129 + 1 + 40_001 + 30_000 + 5 + 1015
    out = np.zeros(4, dtype=graph.SYN_DTYPE)
    for name, s in _invalid_specs().items():
        assert lib.abnn_graph_records(C.byref(s)) == 0, name
        assert graph.records(s) == 0, name
        assert lib.abnn_graph_fill_host(C.byref(s), 0, 1, out.ctypes.data) == 1, name  # ABNN_ERR_INVALID
        with pytest.raises(ValueError):
            graph.reference(s)
    assert lib.abnn_graph_records(None) == 0 == graph.records(None)
    assert not out.view(np.uint32).any()
    with pytest.raises(ValueError):
        graph.spec([graph.dense((0, 2), (2, 2), graph.uniform(0.0, 1.0))] * 17)
    # recipe(): the shape of build_random_graph
    r = graph.recipe(256, 256, 9488, 100_000, seed=9)
    assert (r.seed, r.n_blocks, graph.records(r)) == (9, 2, 100_000)
    d, h = r.blocks[0], r.blocks[1]
    assert (d.count, d.src_first, d.src_count, d.dst_first, d.dst_count, d.topology) == (65_536, 0, 256, 256, 256, 0)
    assert (h.count, h.src_first, h.src_count, h.dst_first, h.dst_count, h.topology) == (34_464, 512, 9488, 512, 9488, 1)
    assert (F32(d.w_lo), F32(d.w_hi), F32(h.w_lo), F32(h.w_hi)) == (F32(0.4), F32(0.8), F32(0.1), F32(0.2))
    assert graph.records(graph.recipe(256, 256, 9488, 1000)) == 1000  # a prefix of the dense block alone


def _fill(s, first, n):
    from abnn_amd import _lib, graph

    out = np.zeros(n + 2, dtype=graph.SYN_DTYPE)  # a guard record on either side
    words = out.view(np.uint32).reshape(-1, 4)
    words[0] = words[-1] = 0xA5A5A5A5
    st = _lib.load().abnn_graph_fill_host(C.byref(s), first, n, out[1:].ctypes.data)
    assert st == 0, (first, n, st)
    assert (words[0] == 0xA5A5A5A5).all() and (words[-1] == 0xA5A5A5A5).all()
    return out[1:-1]


def test_fill_host_equals_the_numpy_rule():
    from abnn_amd import _lib, graph

    s = _mixed_spec()
    total = graph.records(s)
    ref = graph.reference(s)
    assert ref.dtype == graph.SYN_DTYPE and ref.shape == (total,) and not ref["pad"].any()
    got = _fill(s, 0, total)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    # odd sub-ranges that straddle block boundaries, a one-record range, an empty one at the end
    for first, n in ((127, 5), (129, 1), (128, 3), (40_129, 7), (70_125, 13), (70_133, 1018), (1, total - 2), (total, 0),
                     (total - 1, 1)):
        assert np.array_equal(_fill(s, first, n).view(np.uint32), ref[first:first + n].view(np.uint32)), (first, n)
        assert np.array_equal(graph.reference(s, first, n).view(np.uint32), ref[first:first + n].view(np.uint32))
    lib = _lib.load()
    out = np.zeros(4, dtype=graph.SYN_DTYPE)
    for first, n in ((total, 1), (total + 1, 0), (0, total + 1), (1 << 63, 1 << 63), ((1 << 64) - 1, 2)):
        assert lib.abnn_graph_fill_host(C.byref(s), first, n, out.ctypes.data) == 1, (first, n)
    with pytest.raises(ValueError):
        graph.reference(s, total, 1)
    # the populations: every src and dst inside its block's ranges; RANDOM uses both ends of them
    at = 0
    for j in range(s.n_blocks):
        b = s.blocks[j]
        part = ref[at:at + b.count]
        assert part["src"].min() >= b.src_first and part["src"].max() < b.src_first + b.src_count, j
        assert part["dst"].min() >= b.dst_first and part["dst"].max() < b.dst_first + b.dst_count, j
        assert part["w"].min() >= F32(b.w_lo) and part["w"].max() <= F32(b.w_hi), j
        at += b.count
    hid = ref[130:40_131]
    assert hid["src"].min() < 24 + 10 and hid["src"].max() >= 24 + 4072 - 10
    # a block's records depend on its number and the seed alone, not on what the blocks before it hold
    alone = graph.spec([graph.dense((0, 16), (16, 8), graph.uniform(0.4, 0.8), count=5),
                        graph.random((24, 100), (30, 7), 1, graph.beta(2, 8))], s.seed)
    assert np.array_equal(graph.reference(alone)[5:].view(np.uint32), ref[129:130].view(np.uint32))
    # record indices at and above 2^32 within a block: the 64-bit divisions
    big = graph.spec([graph.dense((0, 1000), (1000, 777), graph.uniform(0.0, 1.0), count=(1 << 40)),
                      graph.small_world((0, 1 << 20), 999, 0.25, graph.beta(2, 8), count=(1 << 41))], 77)
    for first in ((1 << 32) - 3, (1 << 39) + 12_345, (1 << 40) - 2, (1 << 40) + (1 << 32) - 5, (1 << 41) + (1 << 40) - 9):
        want = graph.reference(big, first, 9)
        assert np.array_equal(_fill(big, first, 9).view(np.uint32), want.view(np.uint32)), first
    r = (1 << 39) + 12_345
    rec = graph.reference(big, r, 1)[0]
    assert (rec["src"], rec["dst"]) == ((r // 777) % 1000, 1000 + r % 777)


def test_hand_written_six_records():
    """DENSE 2 x 2 (neurons 0, 1 -> 2, 3), then RING n = 5 (neurons 4..8), k = 2,
    p = 0, cut after its first two records: in node numbers 0->1, 0->4."""
    from abnn_amd import graph

    u = graph.uniform(0.5, 1.5)
    s = graph.spec([graph.dense((0, 2), (2, 2), u), graph.small_world((4, 5), 2, 0.0, u, count=2)], 3)
    assert graph.records(s) == 6
    want = [(0, 2), (0, 3), (1, 2), (1, 3), (4 + 0, 4 + 1), (4 + 0, 4 + 4)]
    for rec in (graph.reference(s), _fill(s, 0, 6)):
        assert list(zip(rec["src"].tolist(), rec["dst"].tolist())) == want
        assert ((rec["w"] >= F32(0.5)) & (rec["w"] < F32(1.5))).all() and not rec["pad"].any()
    # the ring's first three nodes on their own: 0->1, 0->4, 1->2, 1->0, 2->3, 2->1
    ring = graph.spec([graph.small_world((0, 5), 2, 0.0, u, count=6)], 3)
    want = [(0, 1), (0, 4), (1, 2), (1, 0), (2, 3), (2, 1)]
    for rec in (graph.reference(ring), _fill(ring, 0, 6)):
        assert list(zip(rec["src"].tolist(), rec["dst"].tolist())) == want
    # a weight by hand: record 0 of block 0, w = w_lo + unit24(X(2)) * (w_hi - w_lo)
    m = (1 << 64) - 1
    z = ((3 ^ (0xD1B54A32D192ED03 * 1)) + (2 + 1) * 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    z ^= z >> 31
    v = F32(z >> 40) * F32(2.0 ** -24)
    assert graph.reference(s)["w"][0] == F32(0.5) + F32(v * (F32(1.5) - F32(0.5)))


@pytest.mark.parametrize("n,k", [(7, 1), (7, 2), (11, 5), (7, 6), (64, 63), (1000, 5)])
def test_ring_lattice_degrees(n, k):
    from abnn_amd import degree, graph

    first = 3
    s = graph.spec([graph.small_world((first, n), k, 0.0, graph.uniform(0.0, 1.0))], 11)
    assert graph.records(s) == n * k
    for rec in (graph.reference(s), _fill(s, 0, n * k)):
        d = degree.reference(rec, degree.config((first, n), ("out", "in")), first + n + 2)
        assert d["out"].tolist() == [k] * n and d["in"].tolist() == [k] * n
        assert (rec["src"] != rec["dst"]).all()
        assert len(set(zip(rec["src"].tolist(), rec["dst"].tolist()))) == n * k  # k distinct neighbours each
    full = graph.spec([graph.small_world((first, n), k, 1.0, graph.uniform(0.0, 1.0), count=4 * n * k + 1)], 12)
    for rec in (graph.reference(full), _fill(full, 0, 4 * n * k + 1)):
        assert (rec["src"] != rec["dst"]).all()
        assert rec["dst"].min() >= first and rec["dst"].max() < first + n
        out = np.bincount(rec["src"] - first, minlength=n)
        assert out.max() - out.min() <= k  # src still walks the ring: 4 k or 4 k + (the wrapped part) each
    if n > 2:
        assert len(np.unique(graph.reference(full)["dst"])) > 1


def test_beta_law():
    from abnn_amd import graph

    n = 200_000
    a, b = 2, 8
    s = graph.spec([graph.random((0, 100), (0, 100), n, graph.beta(a, b))], 2024)
    w = _fill(s, 0, n)["w"]
    assert np.array_equal(w.view(np.uint32), graph.reference(s)["w"].view(np.uint32))
    assert (w >= F32(0.0)).all() and (w < F32(1.0)).all()
    var = a * b / ((a + b) ** 2 * (a + b + 1))  # Var of Beta(a, b)
    se = (var / n) ** 0.5
    # the 24-bit truncation of each draw lowers the mean by less than 2^-24, far below se
    assert abs(float(w.astype(np.float64).mean()) - a / (a + b)) < 6 * se
    # beta(1, 1) is one draw, u(2): the UNIFORM law's v on the same draws
    one = graph.spec([graph.random((0, 100), (0, 100), 5000, graph.beta(1, 1, 0.1, 0.2))], 5)
    uni = graph.spec([graph.random((0, 100), (0, 100), 5000, graph.uniform(0.1, 0.2))], 5)
    assert np.array_equal(_fill(one, 0, 5000).view(np.uint32), _fill(uni, 0, 5000).view(np.uint32))
    assert np.array_equal(graph.reference(one).view(np.uint32), graph.reference(uni).view(np.uint32))
    # laws that keep the largest draws (a > b), fifteen draws, and the extremes
    for (pa, pb) in ((9, 3), (3, 9), (8, 8), (15, 1), (1, 15)):
        sp = graph.spec([graph.random((0, 100), (0, 100), 3000, graph.beta(pa, pb))], 6)
        got = _fill(sp, 0, 3000)["w"]
        assert np.array_equal(got.view(np.uint32), graph.reference(sp)["w"].view(np.uint32)), (pa, pb)
        assert abs(float(got.mean()) - pa / (pa + pb)) < 6 * (pa * pb / ((pa + pb) ** 2 * (pa + pb + 1)) / 3000) ** 0.5


def test_graph_null_arguments_are_invalid_without_a_gpu():
    from abnn_amd import _lib, graph

    lib = _lib.load()
    s = _mixed_spec()
    out = np.zeros(4, dtype=graph.SYN_DTYPE)
    assert lib.abnn_build_graph(None, C.byref(s)) == 1  # ABNN_ERR_INVALID
    assert lib.abnn_build_graph(None, None) == 1
    assert lib.abnn_graph_fill_host(None, 0, 1, out.ctypes.data) == 1
    assert lib.abnn_graph_fill_host(C.byref(s), 0, 1, None) == 1
    assert lib.abnn_graph_fill_host(C.byref(s), 0, 0, None) == 0  # nothing to write
    assert not out.view(np.uint32).any()
