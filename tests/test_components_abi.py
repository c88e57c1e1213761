"""CPU checks of the connected components' boundary (abnn.h abnn_components_*):
the ctypes mirror matches the C layout, abnn_components_words against
components.n_words on valid and invalid configs, null handles without a GPU,
abnn_components_host against the numpy restatement (components.reference) on
seeded records with planted specials, the three-way merge, the host rule under
the sanitizers, and known answers on test_hops_abi.py's hand-made array."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NONE = 0xFFFFFFFF
N = NONE  # ABNN_COMP_NONE
INF = float("inf")
SYN = [("src", "<u4"), ("dst", "<u4"), ("w", "<f4"), ("pad", "<f4")]
# the special weights of tests/test_hops_gpu.py
SPECIAL = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-40, 127.99999, 128.0, -128.0, -127.99999, 0.001, 2.0 ** -24,
                    2.0 ** -25, -(2.0 ** -24)], dtype=F32)


def test_components_config_layout_matches_c(tmp_path):
    from abnn_amd import _lib

    fields = [n for n, _ in _lib.ComponentsConfig._fields_]
    consts = ["ABNN_COMP_WEIGHT", "ABNN_COMP_SIZES", "ABNN_COMP_HEADER_WORDS", "ABNN_COMP_SIZE_BINS", "ABNN_COMP_NONE",
              "ABNN_COMP_BEGIN", "ABNN_COMP_LINK", "ABNN_COMP_FLATTEN", "ABNN_COMP_CLOSE", "ABNN_ABI_VERSION"]
    prog = tmp_path / "sz.c"
    prog.write_text('#include "abnn/abnn.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                    'int main(void){printf("%zu", sizeof(abnn_components_config));\n'
                    + "".join(f'printf(" %llu", (unsigned long long)({c}));\n' for c in consts)
                    + "".join(f'printf(" %zu", offsetof(abnn_components_config, {f}));\n' for f in fields)
                    + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(_lib.ComponentsConfig), _lib.COMP_WEIGHT, _lib.COMP_SIZES, _lib.COMP_HEADER_WORDS, _lib.COMP_SIZE_BINS,
            _lib.COMP_NONE, _lib.COMP_BEGIN, _lib.COMP_LINK, _lib.COMP_FLATTEN, _lib.COMP_CLOSE, _lib.ABI_VERSION,
            *(getattr(_lib.ComponentsConfig, f).offset for f in fields)]
    assert got == want
    assert got[:11] == [32, 1, 2, 8, 32, 0xFFFFFFFF, 0, 1, 2, 3, 10]  # the ABI version stays 10
    assert got[11:] == [0, 4, 8, 12, 16, 20]
    assert fields == ["first", "count", "flags", "w_lo", "w_hi", "reserved"]
    lib = _lib.load()
    for name in ("abnn_components_words", "abnn_components_enqueue", "abnn_components_step_enqueue",
                 "abnn_components_merge_enqueue", "abnn_components", "abnn_components_host"):
        assert hasattr(lib, name) and name in _lib.ABI10_ADDITIONS
    assert hasattr(lib, "abnn_debug_set_components_path")


def _invalid_configs():
    """name -> (config, n_nrn): every refusal abnn.h lists that needs no handle (null is checked apart)."""
    from abnn_amd import components

    bad = {
        "count 0": (components.config((5, 0)), 1000),
        "range ends above n_nrn": (components.config((900, 101)), 1000),
        "first above n_nrn": (components.config((1001, 1)), 1000),
        "range wraps u32": (components.config((0xFFFFFFFF, 2)), 1000),
        "n_nrn 0": (components.config((0, 1)), 0),
        "n_nrn 2^32": (components.config((0, 1)), 1 << 32),
        "w_lo without WEIGHT": (components.config((0, 1)), 1000),
        "w_hi without WEIGHT": (components.config((0, 1)), 1000),
        "-0.0 without WEIGHT": (components.config((0, 1)), 1000),
        "NaN w_lo": (components.config((0, 1), weights=(np.nan, 1.0)), 1000),
        "NaN w_hi": (components.config((0, 1), weights=(0.0, np.nan)), 1000),
        "w_lo == w_hi": (components.config((0, 1), weights=(0.5, 0.5)), 1000),
        "w_lo > w_hi": (components.config((0, 1), weights=(0.5, 0.25)), 1000),
    }
    bad["w_lo without WEIGHT"][0].w_lo = 0.5
    bad["w_hi without WEIGHT"][0].w_hi = 0.5
    bad["-0.0 without WEIGHT"][0].w_lo = -0.0
    for bit in (4, 8, 1 << 31):
        cfg = components.config((0, 1), sizes=True)
        cfg.flags |= bit
        bad[f"flag bit {bit}"] = (cfg, 1000)
    for k in range(3):
        cfg = components.config((0, 10))
        cfg.reserved[k] = 1
        bad[f"reserved[{k}]"] = (cfg, 1000)
    return bad


def test_components_words():
    from abnn_amd import _lib, components

    lib = _lib.load()
    empty = np.zeros(0, dtype=SYN)
    for n_nrn in (1000, 5_000_512, 1001, 1):
        for rng in ((0, 1), (n_nrn - 1, 1), (n_nrn // 2, n_nrn - n_nrn // 2), (0, n_nrn), None):
            for weights in (None, (0.25, 0.9), (-INF, INF)):
                for sizes in (False, True):
                    cfg = components.config(rng, weights, sizes, n_nrn)
                    want = 8 + 32 + (n_nrn + 1) // 2 * (2 if sizes else 1)
                    assert lib.abnn_components_words(C.byref(cfg), n_nrn) == want == components.n_words(cfg, n_nrn), (n_nrn, rng)
    assert components.n_words(components.config(n_nrn=5_000_512), 5_000_512) == 40 + 2_500_256
    out = np.zeros(64, dtype=np.uint64)
    for name, (cfg, n_nrn) in _invalid_configs().items():
        assert lib.abnn_components_words(C.byref(cfg), n_nrn) == 0, name
        assert components.n_words(cfg, n_nrn) == 0 and not components.config_ok(cfg, n_nrn), name
        with pytest.raises(ValueError):
            components.reference(empty, cfg, n_nrn)
        assert lib.abnn_components_host(None, 0, C.byref(cfg), n_nrn, out.ctypes.data, 45) == 1, name
    assert lib.abnn_components_words(None, 1000) == 0
    cfg = components.config((3, 4), weights=(0.25, 0.5), sizes=True)
    assert (cfg.first, cfg.count, cfg.flags, cfg.w_lo, cfg.w_hi, list(cfg.reserved)) == (3, 4, 3, 0.25, 0.5, [0, 0, 0])
    assert components.config((3, 4)).flags == 0
    with pytest.raises(ValueError):
        components.config()  # every neuron: needs n_nrn
    assert (components.BEGIN, components.LINK, components.FLATTEN, components.CLOSE) == (0, 1, 2, 3)
    assert components.NONE == 0xFFFFFFFF and components.PLANE_AT == 40


def test_components_null_arguments_are_invalid_without_a_gpu():
    from abnn_amd import _lib, components

    lib = _lib.load()
    cfg = components.config((0, 4))
    words = components.n_words(cfg, 10)
    out = (C.c_uint64 * words)()
    planes = (C.c_uint32 * 10)()
    assert lib.abnn_components_enqueue(None, C.byref(cfg), out, None) == 1  # ABNN_ERR_INVALID
    for step in (0, 1, 2, 3, 4):
        assert lib.abnn_components_step_enqueue(None, C.byref(cfg), step, out, None) == 1
    assert lib.abnn_components_merge_enqueue(None, C.byref(cfg), planes, 1, out, None) == 1
    assert lib.abnn_components(None, C.byref(cfg), out, words) == 1
    assert lib.abnn_components(None, None, None, 0) == 1
    assert lib.abnn_debug_set_components_path(None, 0) == 1
    # the host rule: null records only with n == 0, the words must match
    syn = np.zeros(3, dtype=SYN)
    assert lib.abnn_components_host(None, 3, C.byref(cfg), 10, out, words) == 1
    assert lib.abnn_components_host(syn.ctypes.data, 3, None, 10, out, words) == 1
    assert lib.abnn_components_host(syn.ctypes.data, 3, C.byref(cfg), 10, None, words) == 1
    assert lib.abnn_components_host(syn.ctypes.data, 3, C.byref(cfg), 10, out, words + 1) == 1
    assert lib.abnn_components_host(None, 0, C.byref(cfg), 10, out, words) == 0


def _host(syn, cfg, n_nrn):
    from abnn_amd import _lib, components

    words = components.n_words(cfg, n_nrn)
    out = np.zeros(words, dtype=np.uint64)
    syn = np.ascontiguousarray(syn)
    st = _lib.load().abnn_components_host(syn.ctypes.data if len(syn) else None, len(syn), C.byref(cfg), n_nrn,
                                          out.ctypes.data, words)
    assert st == 0
    return out


def _records(n, seed, n_nrn=1000, density=1.0):
    """Seeded records as tests/test_hops_gpu.py plants them: uniform src / dst,
    weights in [-0.1, 1.1], the special weights at the first, a middle and the
    last index; then tombstones, ids that are no neuron and self-loops."""
    rng = np.random.default_rng(seed)
    syn = np.zeros(n, dtype=SYN)
    span = max(2, int(n_nrn * density))
    syn["src"] = rng.integers(0, span, n, dtype=np.uint32)
    syn["dst"] = rng.integers(0, span, n, dtype=np.uint32)
    syn["w"] = rng.uniform(-0.1, 1.1, n).astype(F32)
    k = len(SPECIAL)
    if n >= 3 * k:
        for at in (0, n // 2 - k // 2, n - k):
            syn["w"][at:at + k] = SPECIAL
    elif n:
        for j, at in enumerate(sorted({0, n // 2, n - 1})):
            syn["w"][at] = SPECIAL[(seed + j) % k]
    if n >= 20:
        at = rng.choice(n, 8, replace=False)
        syn["src"][at[:2]] = NONE
        syn["dst"][at[:2]] = NONE          # tombstones
        syn["dst"][at[2]] = n_nrn          # dst == N_NRN
        syn["src"][at[3]] = n_nrn          # src == N_NRN
        syn["src"][at[4]] = 0xFFFFFFFE     # a src that is no neuron on a live record
        syn["dst"][at[5]] = syn["src"][at[5]]  # a self-loop
        syn["src"][at[6]], syn["dst"][at[6]] = n_nrn - 1, 0  # the last valid id
    return syn


@pytest.mark.parametrize("seed", range(6))
def test_host_rule_equals_the_numpy_reference(seed):
    from abnn_amd import components

    n_nrn = [1000, 1001, 257, 64, 5000, 2][seed]
    n = [3000, 700, 40, 900, 2500, 50][seed]  # sparse and dense: many components and one
    syn = _records(n, seed, n_nrn)
    for rng in (None, (n_nrn // 3, n_nrn // 2), (n_nrn - 1, 1)):
        for weights in (None, (0.25, 0.9), (-INF, INF), (0.999, INF)):
            for sizes in (False, True):
                cfg = components.config(rng, weights, sizes, n_nrn)
                want = components.reference(syn, cfg, n_nrn)
                got = _host(syn, cfg, n_nrn)
                assert np.array_equal(got, components.to_words(want)), (seed, rng, weights, sizes)
                assert want["followed"] == int(components.followed(syn, cfg, n_nrn).sum())
                back = components.decode(got, cfg, n_nrn)
                assert set(back) == set(want)
                for k, v in want.items():
                    assert np.array_equal(back[k], v) and np.asarray(back[k]).dtype == np.asarray(v).dtype, k
                lab = want["labels"]
                lo, hi = cfg.first, cfg.first + cfg.count
                assert (lab[:lo] == NONE).all() and (lab[hi:] == NONE).all() and (lab[lo:hi] <= np.arange(lo, hi)).all()
                assert int(want["bins"].sum()) == want["components"] and int(want["bins"][0]) == want["singletons"]
                assert want["gave_up"] == 0
    if seed == 0:  # [-inf, inf) leaves out exactly the NaN and the +inf weights, planted three times each
        a = components.reference(syn, components.config(None, None, n_nrn=n_nrn), n_nrn)
        b = components.reference(syn, components.config(None, (-INF, INF), n_nrn=n_nrn), n_nrn)
        assert a["followed"] - b["followed"] == 6


@pytest.mark.parametrize("seed", range(4))
def test_three_way_merge_equals_the_whole(seed):
    from abnn_amd import components

    n_nrn, n = 600, [500, 900, 300, 2000][seed]
    syn = _records(n, 10 + seed, n_nrn)
    for rng, weights in ((None, None), ((100, 400), (0.2, 0.8)), ((0, 300), None)):
        cfg = components.config(rng, weights, True, n_nrn)
        whole = components.reference(syn, cfg, n_nrn)
        parts = [syn[0::3], syn[1::3], syn[2::3]]
        each = [components.reference(p, cfg, n_nrn) for p in parts]
        labels = components.merge([e["labels"] for e in each], cfg)
        merged = components.close(labels, cfg, len(syn), sum(e["followed"] for e in each))
        assert np.array_equal(components.to_words(merged), components.to_words(whole)), (seed, rng)
        assert max(e["components"] for e in each) >= whole["components"]
        # merging a plane into itself changes nothing; entries that are NONE or no neuron of R are skipped
        assert np.array_equal(components.merge([whole["labels"]], cfg), whole["labels"])
        junk = np.full(n_nrn, NONE, dtype=np.uint32)
        junk[::2] = n_nrn + 7
        assert np.array_equal(components.merge([whole["labels"], junk], cfg), whole["labels"])
    with pytest.raises(ValueError):
        components.merge([], components.config((0, 3)))
    with pytest.raises(ValueError):
        components.merge([np.zeros(3, dtype=np.uint32), np.zeros(4, dtype=np.uint32)], components.config((0, 3)))


def test_chain_split_by_parity_merges_into_one():
    """Even-numbered edges of a chain in one part, odd-numbered in the other:
    each alone N / 2 pieces, together one."""
    from abnn_amd import components

    n_nrn = 1000
    syn = np.zeros(n_nrn - 1, dtype=SYN)
    syn["src"] = np.arange(n_nrn - 1)
    syn["dst"] = np.arange(n_nrn - 1) + 1
    syn["w"] = 0.5
    cfg = components.config(n_nrn=n_nrn)
    even, odd = components.reference(syn[0::2], cfg, n_nrn), components.reference(syn[1::2], cfg, n_nrn)
    assert even["components"] == n_nrn // 2 and odd["components"] == n_nrn // 2 + 1
    labels = components.merge([even["labels"], odd["labels"]], cfg)
    assert not labels.any()
    got = components.close(labels, cfg, len(syn), len(syn))
    assert (got["components"], got["largest"], got["largest_label"], got["singletons"]) == (1, n_nrn, 0, 0)
    assert np.array_equal(_host(syn[::-1], cfg, n_nrn), components.to_words(got))  # descending order: the same words


def test_host_rule_under_the_sanitizers(tmp_path):
    """components.h alone, compiled with -fsanitize=address,undefined: a
    stand-alone CPU program over a file of cases; it must exit 0 and give the
    reference's words."""
    from abnn_amd import components
    from abnn_amd.build import build_components_host_test

    prog = build_components_host_test()
    cases = []
    for seed, (n_nrn, n) in enumerate(((1000, 3000), (1001, 64), (1, 5), (2, 0), (333, 4097))):
        syn = _records(n, 20 + seed, n_nrn)
        for rng, weights, sizes in ((None, None, False), (None, (0.25, 0.9), True), ((n_nrn - 1, 1), None, True),
                                    ((n_nrn // 2, n_nrn - n_nrn // 2), (-INF, 0.5), False)):
            cases.append((components.config(rng, weights, sizes, n_nrn), n_nrn, syn))
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(np.uint64(len(cases)).tobytes())
        for cfg, n_nrn, syn in cases:
            f.write(bytes(cfg))
            f.write(np.array([n_nrn, len(syn)], dtype=np.uint64).tobytes())
            f.write(syn.tobytes())
    r = subprocess.run([prog, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    got = np.fromfile(fout, dtype=np.uint64)
    at = 0
    for cfg, n_nrn, syn in cases:
        words = components.n_words(cfg, n_nrn)
        assert np.array_equal(got[at:at + words], components.to_words(components.reference(syn, cfg, n_nrn))), (n_nrn, len(syn))
        at += words
    assert at == len(got)


# (range, weights) -> followed, labels, components / largest / label / singletons, bins 0..3: worked out by hand
HAND = [
    (((0, 10), None), 12, [0, 0, 0, 0, 0, 0, 0, 0, 0, 9], (2, 9, 0, 1), [1, 0, 0, 1]),
    (((0, 10), (0.25, 0.9)), 10, [0, 0, 0, 0, 0, 0, 6, 7, 0, 9], (4, 7, 0, 3), [3, 0, 1, 0]),
    (((3, 5), None), 6, [N, N, N, 3, 3, 3, 3, 3, N, N], (1, 5, 3, 0), [0, 0, 1, 0]),
    (((3, 5), (0.5, INF)), 5, [N, N, N, 3, 3, 3, 6, 3, N, N], (2, 4, 3, 1), [1, 0, 1, 0]),
    (((9, 1), None), 0, [N, N, N, N, N, N, N, N, N, 9], (1, 1, 9, 1), [1, 0, 0, 0]),
]


@pytest.mark.parametrize("case", range(len(HAND)))
def test_known_answers_on_the_hand_made_array(case):
    from abnn_amd import components
    from test_hops_abi import _hand_made

    (rng, weights), n_followed, labels, counts, bins = HAND[case]
    syn = _hand_made()
    assert len(syn) == 15
    for sizes in (False, True):
        cfg = components.config(rng, weights, sizes)
        got = components.reference(syn, cfg, 10)
        assert got["followed"] == n_followed and got["labels"].tolist() == labels
        assert (got["components"], got["largest"], got["largest_label"], got["singletons"]) == counts
        assert got["bins"][:4].tolist() == bins and not got["bins"][4:].any()
        assert (got["records"], got["neurons"], got["gave_up"]) == (15, 10, 0)
        words = components.to_words(got)
        assert words.dtype == np.uint64 and words.shape == (components.n_words(cfg, 10),)
        assert words[:8].tolist() == [15, 10, n_followed, *counts, 0]
        assert np.array_equal(_host(syn, cfg, 10), words)
        for order in (np.arange(15)[::-1], np.random.default_rng(case).permutation(15)):  # the order does not matter
            assert np.array_equal(_host(syn[order], cfg, 10), words)
        if sizes:
            lab = np.array(labels)
            want = [0 if x == N else int((lab == x).sum()) for x in labels]
            assert got["sizes"].tolist() == want
