"""CPU checks of the spike correlograms' boundary (abnn.h abnn_corr_*,
abnn_spikes_load): the ctypes mirror matches the C layout, abnn_corr_words on
every mode and every refusal, null arguments without a GPU, abnn_corr_host
against the numpy restatement (abnn_amd.corr) word for word on random small
inputs, a known answer written out by hand, the identities between the modes,
the merge of two halves of the records, and the host rule in a stand-alone
program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from corr_helpers import NONE, SYN, host, random_records, random_rows, table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_NRN = 40
LAGS = (0, 1, 5, 11, 12)
NAN, INF = float("nan"), float("inf")


def test_layout_matches_c(tmp_path):
    from abnn_amd import _lib

    fields = [n for n, _ in _lib.CorrConfig._fields_]
    consts = ["ABNN_CORR_MAX_LAG", "ABNN_CORR_MAX_PAIR_WORDS", "ABNN_CORR_POP", "ABNN_CORR_PAIRS", "ABNN_CORR_SYNAPSES",
              "ABNN_CORR_WEIGHT", "ABNN_CORR_HEADER_WORDS", "ABNN_ABI_VERSION"]
    prog = tmp_path / "sz.c"
    prog.write_text('#include "abnn/abnn.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                    'int main(void){printf("%zu", sizeof(abnn_corr_config));\n'
                    + "".join(f'printf(" %llu", (unsigned long long)({c}));\n' for c in consts)
                    + "".join(f'printf(" %zu", offsetof(abnn_corr_config, {f}));\n' for f in fields)
                    + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(_lib.CorrConfig), _lib.CORR_MAX_LAG, _lib.CORR_MAX_PAIR_WORDS, _lib.CORR_POP, _lib.CORR_PAIRS,
            _lib.CORR_SYNAPSES, _lib.CORR_WEIGHT, _lib.CORR_HEADER_WORDS, _lib.ABI_VERSION,
            *(getattr(_lib.CorrConfig, f).offset for f in fields)]
    assert got == want
    assert got[:9] == [64, 256, 1 << 24, 0, 1, 2, 1, 8, 10]


def _tweak(cfg, **fields):
    for k, v in fields.items():
        setattr(cfg, k, v)
    return cfg


def _invalid_configs():
    from abnn_amd import corr

    res = (C.c_uint32 * 3)
    return {
        "unknown mode": corr.config(3),
        "unknown flag": _tweak(corr.config("pop"), flags=2),
        "max_lag above the cap": corr.config("pop", max_lag=257),
        "A wraps": corr.config("pop", a=(0xFFFFFFFF, 2)),
        "B wraps": corr.config("synapses", b=(0x80000000, 0x80000001)),
        "PAIRS a_count 0": corr.config("pairs", b=(0, 4), max_lag=1),
        "PAIRS b_count 0": corr.config("pairs", a=(0, 4), max_lag=1),
        "PAIRS too many words": corr.config("pairs", a=(0, 4096), b=(0, 4096), max_lag=1),
        "PAIRS one word too many": corr.config("pairs", a=(0, 1 << 12), b=(0, (1 << 12) // 3 + 1), max_lag=1),
        "bounds without the flag": _tweak(corr.config("synapses"), w_hi=1.0),
        "-0.0 without the flag": _tweak(corr.config("synapses"), w_lo=-0.0),
        "NaN w_lo": corr.config("synapses", weights=(NAN, 1.0)),
        "NaN w_hi": corr.config("synapses", weights=(0.0, NAN)),
        "w_lo == w_hi": corr.config("synapses", weights=(0.5, 0.5)),
        "w_lo > w_hi": corr.config("synapses", weights=(0.5, 0.25)),
        "reserved 0": _tweak(corr.config("pop"), reserved=res(1, 0, 0)),
        "reserved 2": _tweak(corr.config("pop"), reserved=res(0, 0, 1)),
    }


def test_corr_words():
    from abnn_amd import _lib, corr

    lib = _lib.load()
    for L in (0, 1, 16, 256):
        for mode in ("pop", "synapses"):
            cfg = corr.config(mode, max_lag=L)
            assert lib.abnn_corr_words(C.byref(cfg)) == 8 + 2 * L + 1 == corr.n_words(cfg)
        cfg = corr.config("pairs", a=(3, 5), b=(10, 7), max_lag=L)
        assert lib.abnn_corr_words(C.byref(cfg)) == 8 + 5 * 7 * (2 * L + 1) == corr.n_words(cfg)
    cfg = corr.config("pairs", a=(0, 1 << 12), b=(0, (1 << 12) // 3), max_lag=1)  # the largest that fits at L = 1
    assert lib.abnn_corr_words(C.byref(cfg)) == 8 + (1 << 12) * ((1 << 12) // 3) * 3 == corr.n_words(cfg)
    cfg = corr.config("synapses", a=(0xFFFFFFFF, 1), weights=(-INF, INF), rows=(1 << 40, 1 << 50))
    assert lib.abnn_corr_words(C.byref(cfg)) == 8 + 33 == corr.n_words(cfg)
    passes, raster = table([])
    out = np.zeros(16, dtype=np.uint64)
    for name, cfg in _invalid_configs().items():
        assert lib.abnn_corr_words(C.byref(cfg)) == 0, name
        assert corr.n_words(cfg) == 0, name
        with pytest.raises(ValueError):
            corr.reference(cfg, N_NRN, passes, raster)
        assert lib.abnn_corr_host(C.byref(cfg), N_NRN, None, 0, None, 0, None, 0, out.ctypes.data) == 1, name
    assert lib.abnn_corr_words(None) == 0
    cfg = corr.config("synapses", a=(1, 2), b=(3, 4), max_lag=7, rows=(5, 6), weights=(0.25, 0.5))
    assert (cfg.a_first, cfg.a_count, cfg.b_first, cfg.b_count, cfg.row_first, cfg.row_count, cfg.max_lag, cfg.mode,
            cfg.flags, cfg.w_lo, cfg.w_hi, list(cfg.reserved)) == (1, 2, 3, 4, 5, 6, 7, 2, 1, 0.25, 0.5, [0, 0, 0])


def test_null_and_range_arguments_are_invalid_without_a_gpu():
    from abnn_amd import _lib, corr

    lib = _lib.load()
    cfg = corr.config("pop", max_lag=1)
    passes, raster = table([[1, 2], [3]])
    out = np.zeros(16, dtype=np.uint64)
    p, r, o = passes.ctypes.data, raster.ctypes.data, out.ctypes.data
    assert lib.abnn_corr_enqueue(None, C.byref(cfg), o, None) == 1  # ABNN_ERR_INVALID
    assert lib.abnn_corr(None, C.byref(cfg), o, 11) == 1
    assert lib.abnn_spikes_load(None, p, 2, r, 3) == 1
    assert lib.abnn_corr_host(None, N_NRN, p, 2, r, 3, None, 0, o) == 1
    assert lib.abnn_corr_host(C.byref(cfg), N_NRN, None, 2, r, 3, None, 0, o) == 1
    assert lib.abnn_corr_host(C.byref(cfg), N_NRN, p, 2, None, 3, None, 0, o) == 1
    assert lib.abnn_corr_host(C.byref(cfg), N_NRN, p, 2, r, 3, None, 5, o) == 1
    assert lib.abnn_corr_host(C.byref(cfg), N_NRN, p, 2, r, 3, None, 0, None) == 1
    for bad in (corr.config("pop", a=(30, 11)), corr.config("pop", b=(40, 1)), corr.config("synapses", a=(0, 41))):
        assert lib.abnn_corr_host(C.byref(bad), N_NRN, p, 2, r, 3, None, 0, o) == 1
    assert lib.abnn_corr_host(C.byref(corr.config("pop", a=(30, 10), max_lag=1)), N_NRN, p, 2, r, 3, None, 0, o) == 0
    assert lib.abnn_corr_host(C.byref(cfg), N_NRN, None, 0, None, 0, None, 0, o) == 0 and not out[:11].any()


def _cases():
    rng = np.random.default_rng(7)
    rows = random_rows(rng, N_NRN, 12, 9)
    rows[3] = rows[3][:0]  # an empty row
    passes, raster = table(rows)
    return passes, raster, random_records(rng, N_NRN, 300)


RANGES = [(None, None), ((0, 10), None), (None, (5, 30)), ((2, 6), (0, 4)), ((39, 1), (0, 40))]


@pytest.mark.parametrize("L", LAGS)
def test_host_rule_equals_the_numpy_restatement(L):
    from abnn_amd import corr

    passes, raster, rec = _cases()
    for a, b in RANGES:
        for rows in (None, (3, 6), (11, 0), (12, 4)):  # all, strictly inside, the last row, past K
            for mode in ("pop", "synapses", "pairs"):
                if mode == "pairs" and (a is None or b is None):
                    a2, b2 = a or (0, N_NRN), b or (0, N_NRN)
                else:
                    a2, b2 = a, b
                for weights in ((None, (0.25, 0.75), (0.5, INF)) if mode == "synapses" else (None,)):
                    cfg = corr.config(mode, a2, b2, L, rows, weights)
                    want = corr.reference(cfg, N_NRN, passes, raster, rec)
                    got = host(cfg, N_NRN, passes, raster, rec if mode == "synapses" else None)
                    assert got.tolist() == corr.to_words(want).tolist(), (mode, a, b, rows, weights)
                    assert want["total"] == int(want["plane"].sum()) and want["recorded"] == 12
                    assert want["rows"] == (12 if rows is None else {3: 6, 11: 1, 12: 0}[rows[0]])
    d = corr.reference(corr.config("synapses", max_lag=L), N_NRN, passes, raster, rec)
    assert 0 < d["coupled"] <= d["followed"] < 300 and d["total"] > 0  # the cases reach what they are for


def test_known_answer_by_hand():
    """Five neurons, four rows.  Row 0: 1 1 2 (id 1 twice); row 1: empty; row 2:
    3; row 3: 1 4.  A = {1, 2}, B = {1, 2, 3, 4}, L = 3: the pairs at lag +3 (row 0
    -> row 3) and at -3 (row 3 -> row 0) lie exactly on the edge."""
    from abnn_amd import corr

    passes, raster = table([[1, 1, 2], [], [3], [1, 4]])
    # per row: entries in A = 3 0 0 1, in B = 3 0 1 2
    cfg = corr.config("pop", a=(1, 2), b=(1, 4), max_lag=3)
    got = host(cfg, 5, passes, raster)
    #        lag -3: A row 3 x B row 0 = 1*3;  -2: none (A rows 2, 3 x B rows 0, 1);  -1: A3 x B2 = 1
    #        lag  0: 3*3 + 1*2 = 11;  +1: none;  +2: A0 x B2 = 3;  +3: A0 x B3 = 3*2 = 6
    assert got.tolist() == [4, 6, 4, 6, 24, 0, 0, 4, 3, 0, 1, 11, 0, 3, 6]
    assert corr.to_words(corr.reference(cfg, 5, passes, raster)).tolist() == got.tolist()
    # with L = 2 the two edge bins fall away, nothing else moves
    cfg = corr.config("pop", a=(1, 2), b=(1, 4), max_lag=2)
    assert host(cfg, 5, passes, raster).tolist() == [4, 6, 4, 6, 15, 0, 0, 4, 0, 1, 11, 0, 3]
    # records: 1 -> 1 (self: row 0 twice, row 3), 2 -> 4, 1 -> 3, a tombstone, 3 -> 1 (src outside A),
    # 2 -> 3 with w = NaN (followed without the weight flag)
    rec = np.array([(1, 1, 0.5, 0), (2, 4, 0.5, 0), (1, 3, 0.25, 0), (NONE, NONE, 0.5, 0), (3, 1, 0.5, 0),
                    (2, 3, np.nan, 0)], dtype=SYN)
    cfg = corr.config("synapses", a=(1, 2), b=(1, 4), max_lag=3)
    got = host(cfg, 5, passes, raster, rec)
    # 1 -> 1: lists {0, 0, 3} x {0, 0, 3}: lag 0: 2*2 + 1 = 5, +3: 2, -3: 2
    # 2 -> 4: {0} x {3}: +3: 1;  1 -> 3: {0, 0, 3} x {2}: +2: 2, -1: 1;  2 -> 3: {0} x {2}: +2: 1
    assert got.tolist() == [4, 6, 4, 6, 14, 4, 4, 4, 2, 0, 1, 5, 0, 3, 3]
    assert corr.to_words(corr.reference(cfg, 5, passes, raster, rec)).tolist() == got.tolist()
    cfg = corr.config("synapses", a=(1, 2), b=(1, 4), max_lag=3, weights=(0.5, 1.0))  # drops 1 -> 3 and the NaN
    got = host(cfg, 5, passes, raster, rec)
    assert got.tolist() == [4, 6, 4, 6, 10, 2, 2, 4, 2, 0, 0, 5, 0, 0, 3]
    # the PAIRS cell of (1, 1)
    cfg = corr.config("pairs", a=(1, 1), b=(1, 1), max_lag=3)
    assert host(cfg, 5, passes, raster).tolist() == [4, 6, 3, 3, 9, 0, 0, 4, 2, 0, 0, 5, 0, 0, 2]


@pytest.mark.parametrize("L", LAGS)
def test_identities(L):
    from abnn_amd import corr

    passes, raster, rec = _cases()
    sym = corr.decode(host(corr.config("pop", (3, 20), (3, 20), L), N_NRN, passes, raster), corr.config("pop", (3, 20), (3, 20), L))
    assert sym["plane"].tolist() == sym["plane"][::-1].tolist() and sym["total"] > 0  # A = B: symmetric in the lag
    cfg_all = corr.config("pairs", (0, N_NRN), (0, N_NRN), L)
    m = corr.decode(host(cfg_all, N_NRN, passes, raster), cfg_all)
    for a, b in RANGES:
        pop = corr.decode(host(corr.config("pop", a, b, L), N_NRN, passes, raster), corr.config("pop", a, b, L))
        af, ac = a or (0, N_NRN)
        bf, bc = b or (0, N_NRN)
        assert m["plane"][af:af + ac, bf:bf + bc].sum(axis=(0, 1)).tolist() == pop["plane"].tolist()
        assert pop["total"] == int(pop["plane"].sum())
        cfg = corr.config("synapses", a, b, L, weights=(0.25, INF))
        syn = corr.decode(host(cfg, N_NRN, passes, raster, rec), cfg)
        keep = (rec["dst"] != NONE) & (rec["w"] >= np.float32(0.25))
        keep &= (rec["src"] - np.uint32(af) < ac) & (rec["dst"] - np.uint32(bf) < bc)
        s, t = rec["src"][keep].astype(np.int64), rec["dst"][keep].astype(np.int64)
        assert m["plane"][s, t].sum(axis=0).tolist() == syn["plane"].tolist()
        assert syn["followed"] == int(keep.sum()) and syn["total"] == int(syn["plane"].sum())
        assert syn["coupled"] == int((m["plane"][s, t].sum(axis=1) > 0).sum())
    assert m["total"] == int(m["plane"].sum())


def test_merge_of_two_halves():
    from abnn_amd import corr

    passes, raster, rec = _cases()
    for a, b, weights in ((None, None, None), ((0, 20), (10, 30), (0.1, 0.9))):
        cfg = corr.config("synapses", a, b, 5, weights=weights)
        whole = corr.decode(host(cfg, N_NRN, passes, raster, rec), cfg)
        parts = [corr.decode(host(cfg, N_NRN, passes, raster, rec[lo:hi]), cfg) for lo, hi in ((0, 131), (131, 300))]
        assert corr.to_words(corr.merge(parts)).tolist() == corr.to_words(whole).tolist()
    with pytest.raises(ValueError):
        corr.merge([])


def test_host_rule_under_the_sanitizers(tmp_path):
    """csrc/corr.h's host rule in a stand-alone program built with
    -fsanitize=address,undefined: a child process that must exit 0."""
    from abnn_amd.build import build_corr_host_test

    prog = build_corr_host_test(out=str(tmp_path / "corr_host_test"))
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    assert "300 cases ok" in r.stdout
