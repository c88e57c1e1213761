"""CPU checks of the connectivity matrix's boundary (abnn.h abnn_matrix_*): the
ctypes mirror matches the C layout, abnn_matrix_words against matrix.n_words on
valid and invalid configs, null handles and contradictory partitions without a
GPU, abnn_matrix_host against the numpy restatement (matrix.reference) on
seeded records with planted specials, the identities of the rule, the three-way
merge, the two's-complement wrap, the host rule under the sanitizers, and tables
worked out by hand on test_hops_abi.py's hand-made array."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from test_components_abi import SPECIAL, SYN, _records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NONE = 0xFFFFFFFF
INF = float("inf")
BASE = 0.8  # abnn_params.base_scale's default
WHATS = [tuple(k for k, on in zip(("count", "w", "p"), bits) if on) for bits in itertools.product((0, 1), repeat=3)][1:]
POPS = (1, 2, 3, 63, 64)


def test_matrix_config_layout_matches_c(tmp_path):
    from abnn_amd import _lib

    fields = [n for n, _ in _lib.MatrixConfig._fields_]
    consts = ["ABNN_MAT_COUNT", "ABNN_MAT_W", "ABNN_MAT_P", "ABNN_MAT_LABELS", "ABNN_MAT_WEIGHT", "ABNN_MATRIX_MAX_POPS",
              "ABNN_MATRIX_HEADER_WORDS", "ABNN_ABI_VERSION"]
    prog = tmp_path / "sz.c"
    prog.write_text('#include "abnn/abnn.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                    'int main(void){printf("%zu", sizeof(abnn_matrix_config));\n'
                    + "".join(f'printf(" %llu", (unsigned long long)({c}));\n' for c in consts)
                    + "".join(f'printf(" %zu", offsetof(abnn_matrix_config, {f}));\n' for f in fields)
                    + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(_lib.MatrixConfig), _lib.MAT_COUNT, _lib.MAT_W, _lib.MAT_P, _lib.MAT_LABELS, _lib.MAT_WEIGHT,
            _lib.MATRIX_MAX_POPS, _lib.MATRIX_HEADER_WORDS, _lib.ABI_VERSION, *(getattr(_lib.MatrixConfig, f).offset for f in fields)]
    assert got == want
    assert got[:9] == [32, 1, 2, 4, 1, 2, 64, 16, 10]  # the ABI version stays 10
    assert got[9:] == [0, 4, 8, 12, 16, 20]
    assert fields == ["pops", "what", "flags", "w_lo", "w_hi", "reserved"]
    lib = _lib.load()
    for name in ("abnn_matrix_words", "abnn_matrix_enqueue", "abnn_matrix", "abnn_matrix_host"):
        assert hasattr(lib, name) and name in _lib.ABI10_ADDITIONS
    assert hasattr(lib, "abnn_debug_set_matrix_path")


def _invalid_configs():
    """name -> config: every refusal of abnn_matrix_words."""
    from abnn_amd import matrix

    bad = {
        "pops 0": matrix.config(0),
        "pops 65": matrix.config(65),
        "pops 2^32 - 1": matrix.config(0xFFFFFFFF),
        "what empty": matrix.config(3, ()),
        "w_lo without WEIGHT": matrix.config(3),
        "w_hi without WEIGHT": matrix.config(3),
        "-0.0 without WEIGHT": matrix.config(3),
        "NaN w_lo": matrix.config(3, weights=(np.nan, 1.0)),
        "NaN w_hi": matrix.config(3, weights=(0.0, np.nan)),
        "w_lo == w_hi": matrix.config(3, weights=(0.5, 0.5)),
        "w_lo > w_hi": matrix.config(3, weights=(0.5, 0.25)),
    }
    bad["w_lo without WEIGHT"].w_lo = 0.5
    bad["w_hi without WEIGHT"].w_hi = 0.5
    bad["-0.0 without WEIGHT"].w_lo = -0.0
    for bit in (8, 16, 1 << 31):
        bad[f"what bit {bit}"] = matrix.config(3, 1 | bit)
    for bit in (4, 8, 1 << 31):
        cfg = matrix.config(3)
        cfg.flags |= bit
        bad[f"flag bit {bit}"] = cfg
    for k in range(3):
        cfg = matrix.config(3)
        cfg.reserved[k] = 1
        bad[f"reserved[{k}]"] = cfg
    return bad


def _host_status(syn, cfg, n_nrn, bounds=None, labels=None, words=None, out=True):
    from abnn_amd import _lib, matrix

    words = matrix.n_words(cfg) if words is None else words
    res = np.zeros(max(words, 1) + 8, dtype=np.uint64)
    syn = np.ascontiguousarray(syn)
    b = None if bounds is None else np.ascontiguousarray(bounds, dtype=np.uint32)
    lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.uint32)
    st = _lib.load().abnn_matrix_host(syn.ctypes.data if len(syn) else None, len(syn), C.byref(cfg),
                                      None if b is None else b.ctypes.data, None if lab is None else lab.ctypes.data, n_nrn,
                                      BASE, res.ctypes.data if out else None, words)
    assert not res[max(words, 1):].any()  # nothing is written past the words
    return st, res[:words]


def _host(syn, cfg, n_nrn, bounds=None, labels=None):
    st, res = _host_status(syn, cfg, n_nrn, bounds, labels)
    assert st == 0
    return res


def test_matrix_words_and_refusals():
    from abnn_amd import _lib, matrix

    lib = _lib.load()
    empty = np.zeros(0, dtype=SYN)
    for pops in (1, 2, 3, 8, 63, 64):
        for what in WHATS:
            for labels in (False, True):
                for weights in (None, (0.25, 0.9), (-INF, INF)):
                    cfg = matrix.config(pops, what, labels, weights)
                    want = 16 + pops + len(what) * pops * pops
                    assert lib.abnn_matrix_words(C.byref(cfg)) == want == matrix.n_words(cfg), (pops, what)
                    assert matrix.config_ok(cfg) and matrix.n_planes(cfg) == len(what)
    assert matrix.n_words(matrix.config(64, ("count", "w", "p"))) == 16 + 64 + 3 * 4096
    assert matrix.config(3, 5).what == 5 and matrix.config(3, ("p", "count")).what == 5
    ok_bounds = np.array([0, 3, 6, 10], dtype=np.uint32)
    for name, cfg in _invalid_configs().items():
        assert lib.abnn_matrix_words(C.byref(cfg)) == 0, name
        assert matrix.n_words(cfg) == 0 and not matrix.config_ok(cfg), name
        with pytest.raises(ValueError):
            matrix.reference(empty, cfg, 10, BASE, bounds=ok_bounds)
        assert _host_status(empty, cfg, 10, ok_bounds, words=28)[0] == 1, name
    assert lib.abnn_matrix_words(None) == 0
    # the partition: decreasing bounds, bounds[P] > N_NRN, the wrong or both or no partition argument
    cfg = matrix.config(3)
    labels = np.zeros(10, dtype=np.uint32)
    for bounds in ([0, 5, 4, 10], [3, 2, 2, 2], [0, 3, 6, 11], [0, 0, 0, 0xFFFFFFFF], [11, 11, 11, 11]):
        assert not matrix.bounds_ok(bounds, 3, 10)
        assert _host_status(empty, cfg, 10, bounds)[0] == 1, bounds
        with pytest.raises(ValueError):
            matrix.reference(empty, cfg, 10, BASE, bounds=bounds)
    for bounds in ([0, 3, 6, 10], [0, 0, 0, 0], [10, 10, 10, 10], [2, 2, 9, 9]):
        assert matrix.bounds_ok(bounds, 3, 10) and _host_status(empty, cfg, 10, bounds)[0] == 0
    assert not matrix.bounds_ok([0, 3, 10], 3, 10)  # P values
    lcfg = matrix.config(3, labels=True)
    for c, b, lab in ((cfg, None, None), (cfg, None, labels), (cfg, ok_bounds, labels), (lcfg, None, None), (lcfg, ok_bounds, None),
                      (lcfg, ok_bounds, labels)):
        assert _host_status(empty, c, 10, b, lab)[0] == 1
        with pytest.raises(ValueError):
            matrix.reference(empty, c, 10, BASE, bounds=b, labels=lab)
    assert _host_status(empty, lcfg, 10, None, labels)[0] == 0
    for n_nrn in (0, 1 << 32):
        assert _host_status(empty, lcfg, n_nrn, None, labels)[0] == 1
    assert matrix.io_bounds(256, 128, 1000).tolist() == [0, 256, 384, 1384]
    assert matrix.io_bounds(256, 128, 1000).dtype == np.uint32


def test_matrix_null_arguments_are_invalid_without_a_gpu():
    from abnn_amd import _lib, matrix

    lib = _lib.load()
    cfg, lcfg = matrix.config(3), matrix.config(3, labels=True)
    words = matrix.n_words(cfg)
    out = (C.c_uint64 * words)()
    bounds = (C.c_uint32 * 4)(0, 3, 6, 10)
    labels = (C.c_uint32 * 10)()
    assert lib.abnn_matrix_enqueue(None, C.byref(cfg), bounds, None, out, None) == 1  # ABNN_ERR_INVALID
    assert lib.abnn_matrix_enqueue(None, C.byref(lcfg), None, labels, out, None) == 1
    assert lib.abnn_matrix_enqueue(None, C.byref(cfg), bounds, labels, out, None) == 1
    assert lib.abnn_matrix_enqueue(None, None, None, None, None, None) == 1
    assert lib.abnn_matrix(None, C.byref(cfg), bounds, None, out, words) == 1
    assert lib.abnn_matrix(None, C.byref(cfg), None, None, out, words) == 1
    assert lib.abnn_matrix(None, None, None, None, None, 0) == 1
    assert lib.abnn_debug_set_matrix_path(None, 0) == 1
    # the host rule: null records only with n == 0, the words must match
    syn = np.zeros(3, dtype=SYN)
    b = np.array([0, 3, 6, 10], dtype=np.uint32)
    assert lib.abnn_matrix_host(None, 3, C.byref(cfg), b.ctypes.data, None, 10, BASE, out, words) == 1
    assert lib.abnn_matrix_host(syn.ctypes.data, 3, None, b.ctypes.data, None, 10, BASE, out, words) == 1
    assert lib.abnn_matrix_host(syn.ctypes.data, 3, C.byref(cfg), b.ctypes.data, None, 10, BASE, None, words) == 1
    assert lib.abnn_matrix_host(syn.ctypes.data, 3, C.byref(cfg), b.ctypes.data, None, 10, BASE, out, words + 1) == 1
    assert lib.abnn_matrix_host(None, 0, C.byref(cfg), b.ctypes.data, None, 10, BASE, out, words) == 0
    assert list(out)[:12] == [0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 10, 10] and list(out)[16:19] == [3, 3, 4]  # n == 0: the sizes only


def _partitions(pops, n_nrn, seed):
    """(name, bounds, labels): bounds with empty populations, bounds that leave
    a prefix and a suffix unassigned, bounds[0] == bounds[P], and labels that
    hold values >= P, 0xFFFFFFFF and P - 1."""
    rng = np.random.default_rng(1000 * pops + seed)
    cuts = np.sort(rng.integers(0, n_nrn + 1, pops + 1)).astype(np.uint32)
    cuts[0], cuts[-1] = 0, n_nrn
    if pops >= 2:
        cuts[1] = cuts[0]  # an empty population (more where the draws repeat: pops > n_nrn forces them)
    lo = n_nrn // 10 + (n_nrn > 10)
    inner = np.sort(rng.integers(lo, max(lo + 1, n_nrn - n_nrn // 10), pops + 1)).astype(np.uint32)
    point = np.full(pops + 1, n_nrn // 2, dtype=np.uint32)
    labels = rng.integers(0, pops + 2, n_nrn).astype(np.uint32)  # pops and pops + 1: no population
    labels[rng.integers(0, n_nrn, max(1, n_nrn // 20))] = NONE
    labels[[0, n_nrn - 1]] = pops - 1
    return [("cover", cuts, None), ("inner", inner, None), ("point", point, None), ("labels", None, labels)]


def _check_identities(d, what):
    assert (d["tombstones"] + d["counted"] + d["src_unassigned"] + d["dst_unassigned"] + d["unassigned"]
            + d["out_of_band"]) == d["records"]
    assert int(d["sizes"].sum()) == d["assigned"] <= d["neurons"]
    if "count" in what:
        assert int(d["count"].sum()) == d["counted"]
    assert ("w" in what) or d["skipped_w"] == 0
    assert ("p" in what) or d["skipped_p"] == 0


@pytest.mark.parametrize("seed", range(4))
def test_host_rule_equals_the_numpy_reference(seed):
    from abnn_amd import matrix

    n_nrn = [1000, 1001, 257, 64][seed]
    n = [3000, 700, 400, 900][seed]
    syn = _records(n, seed, n_nrn)
    assert np.isin(SPECIAL.view(np.uint32), syn["w"].view(np.uint32)).all()
    assert (syn["dst"] == NONE).any() and (syn["src"] == n_nrn).any() and (syn["dst"] == n_nrn).any()
    assert (syn["src"] == 0xFFFFFFFE).any() and (syn["src"] == n_nrn - 1).any()
    seen_skips = 0
    for pops in POPS:
        for name, bounds, labels in _partitions(pops, n_nrn, seed):
            for what in WHATS:
                for weights in (None, (0.25, 0.9)):
                    cfg = matrix.config(pops, what, labels is not None, weights)
                    want = matrix.reference(syn, cfg, n_nrn, BASE, bounds=bounds, labels=labels)
                    got = _host(syn, cfg, n_nrn, bounds, labels)
                    assert np.array_equal(got, matrix.to_words(want)), (seed, pops, name, what, weights)
                    _check_identities(want, what)
                    back = matrix.decode(got, cfg)
                    for k, v in want.items():
                        assert np.array_equal(back[k], v) and np.asarray(back[k]).dtype == np.asarray(v).dtype, k
                    assert want["pops"] == pops and want["neurons"] == n_nrn and want["records"] == n
                    assert not got[12:16].any()
                    seen_skips += want["skipped_w"] + want["skipped_p"]
                    if name == "point":
                        assert want["assigned"] == 0 and want["counted"] == 0
                    if name == "cover" and weights is None:  # only the ids that are no neuron stay unassigned
                        assert want["src_unassigned"] + want["dst_unassigned"] + want["unassigned"] == 3
    assert seen_skips > 0  # NaN, +-inf and +-128 were counted and not summed somewhere
    # decode's floats and density
    cfg = matrix.config(3, ("count", "w", "p"))
    d = matrix.decode(_host(syn, cfg, n_nrn, matrix.io_bounds(n_nrn // 4, n_nrn // 4, n_nrn - 2 * (n_nrn // 4))), cfg)
    assert np.array_equal(d["w_float"], d["w"] / 2.0 ** 24) and np.array_equal(d["p_float"], d["p"] / 2.0 ** 24)
    assert np.allclose(d["density"], d["count"] / np.outer(d["sizes"], d["sizes"]))


@pytest.mark.parametrize("seed", range(3))
def test_three_way_merge_equals_the_whole(seed):
    from abnn_amd import matrix

    n_nrn, n = 600, [500, 900, 2000][seed]
    syn = _records(n, 10 + seed, n_nrn)
    for pops in (1, 3, 64):
        for name, bounds, labels in _partitions(pops, n_nrn, seed):
            cfg = matrix.config(pops, ("count", "w", "p"), labels is not None, (0.2, 0.8) if seed == 1 else None)
            whole = matrix.reference(syn, cfg, n_nrn, BASE, bounds=bounds, labels=labels)
            each = [matrix.reference(p, cfg, n_nrn, BASE, bounds=bounds, labels=labels) for p in (syn[0::3], syn[1::3], syn[2::3])]
            merged = matrix.merge(each)
            assert np.array_equal(matrix.to_words(merged), matrix.to_words(whole)), (seed, pops, name)
            assert np.array_equal(matrix.merge_words([matrix.to_words(e) for e in each]), matrix.to_words(whole))
    with pytest.raises(ValueError):
        matrix.merge([])
    a = matrix.reference(syn, matrix.config(2), n_nrn, BASE, bounds=[0, 5, 9])
    b = matrix.reference(syn, matrix.config(2), n_nrn, BASE, bounds=[0, 5, 10])
    with pytest.raises(ValueError):
        matrix.merge([a, b])  # different partitions


def test_negative_sums_wrap_as_twos_complement():
    from abnn_amd import matrix

    syn = np.zeros(2, dtype=SYN)
    syn["src"], syn["dst"], syn["w"] = 1, 2, F32(-127.99999)
    q = int(F32(-127.99999) * F32(16777216.0))
    assert -(1 << 31) < q < -(1 << 30)
    cfg = matrix.config(1, ("w", "p"))
    got = _host(syn, cfg, 4, [0, 4])
    assert int(got[17]) == (2 * q) % (1 << 64) and int(got[17]) > 1 << 63  # the word, not a float
    assert got[7] == 0 and got[8] == 2 and got[18] == 0  # (w * w) * 0.8 is far above 128: counted, not summed for P
    want = matrix.reference(syn, cfg, 4, BASE, bounds=[0, 4])
    assert np.array_equal(got, matrix.to_words(want)) and int(want["w"][0, 0]) == 2 * q


def _q(c):
    return int(F32(c) * F32(16777216.0))


def test_tables_worked_out_by_hand():
    from abnn_amd import matrix
    from test_hops_abi import _hand_made

    syn = _hand_made()
    assert len(syn) == 15
    # partition A: [0, 3) [3, 6) [6, 10), no band: records 13 / 14 leave / enter at neuron 10 = N_NRN
    cfg = matrix.config(3, ("count", "w"))
    got = matrix.reference(syn, cfg, 10, BASE, bounds=[0, 3, 6, 10])
    words = matrix.to_words(got)
    assert words[:16].tolist() == [15, 1, 12, 1, 1, 0, 0, 1, 0, 3, 10, 10, 0, 0, 0, 0]  # word 7: the NaN of record 10
    assert got["sizes"].tolist() == [3, 3, 4]
    assert got["count"].tolist() == [[3, 2, 0], [0, 4, 2], [1, 0, 0]]
    half = 1 << 23
    assert got["w"].tolist() == [[2 * half + _q(0.6), 2 * half, 0], [0, 4 * half, _q(0.9)], [half, 0, 0]]
    assert np.array_equal(_host(syn, cfg, 10, [0, 3, 6, 10]), words)
    # partition B: population 0 empty, neurons 0 and 9 unassigned, the band [0.25, 0.9) drops the NaN and the 0.9
    table = [[0, 0, 0], [0, 4, 1], [0, 1, 0]]
    head = [15, 1, 6, 3, 2, 1, 2, 0, 0, 3, 10, 8, 0, 0, 0, 0]
    qp = _q(F32(F32(0.5) * F32(0.5)) * F32(BASE))
    labels = np.array([NONE, 1, 1, 1, 1, 2, 2, 2, 2, 7], dtype=np.uint32)
    for lab, kw in ((False, {"bounds": [1, 1, 5, 9]}), (True, {"labels": labels})):
        cfg = matrix.config(3, ("count", "p"), lab, (0.25, 0.9))
        got = matrix.reference(syn, cfg, 10, BASE, **kw)
        words = matrix.to_words(got)
        assert words[:16].tolist() == head and got["sizes"].tolist() == [0, 4, 4]
        assert got["count"].tolist() == table and got["p"].tolist() == (np.array(table) * qp).tolist()
        assert np.array_equal(_host(syn, cfg, 10, kw.get("bounds"), kw.get("labels")), words)
        for order in (np.arange(15)[::-1], np.random.default_rng(5).permutation(15)):  # the order does not matter
            assert np.array_equal(_host(syn[order], cfg, 10, kw.get("bounds"), kw.get("labels")), words)
        d = matrix.decode(words, cfg)
        assert d["density"][1, 1] == 4 / 16 and np.isnan(d["density"][0, 0])


def test_host_rule_under_the_sanitizers(tmp_path):
    """matrix.h alone, compiled with -fsanitize=address,undefined: a stand-alone
    CPU program over a file of cases; it must exit 0 and give the reference's words."""
    from abnn_amd import matrix
    from abnn_amd.build import build_matrix_host_test

    prog = build_matrix_host_test()
    cases = []
    for seed, (n_nrn, n) in enumerate(((1000, 3000), (1001, 64), (1, 5), (2, 0), (333, 4097))):
        syn = _records(n, 20 + seed, n_nrn)
        for pops in (1, 3, 64):
            for k, (name, bounds, labels) in enumerate(_partitions(pops, n_nrn, seed)):
                cfg = matrix.config(pops, WHATS[(pops + k) % len(WHATS)], labels is not None, (0.25, 0.9) if k % 2 else None)
                cases.append((cfg, n_nrn, syn, bounds, labels))
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(np.uint64(len(cases)).tobytes())
        for cfg, n_nrn, syn, bounds, labels in cases:
            f.write(bytes(cfg))
            f.write(np.array([n_nrn, len(syn)], dtype=np.uint64).tobytes())
            f.write(np.array([BASE, 0.0], dtype=F32).tobytes())
            f.write(np.ascontiguousarray(bounds if labels is None else labels, dtype=np.uint32).tobytes())
            f.write(syn.tobytes())
    r = subprocess.run([prog, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    got = np.fromfile(fout, dtype=np.uint64)
    at = 0
    for cfg, n_nrn, syn, bounds, labels in cases:
        words = matrix.n_words(cfg)
        want = matrix.to_words(matrix.reference(syn, cfg, n_nrn, BASE, bounds=bounds, labels=labels))
        assert np.array_equal(got[at:at + words], want), (n_nrn, len(syn), cfg.pops)
        at += words
    assert at == len(got)
