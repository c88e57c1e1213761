"""CPU checks of the snapshots' boundary (abnn.h abnn_snapshot_*): the ctypes
mirrors match the C layouts, abnn_snapshot_diff_words against snapshot.n_words
on valid configs and on every refusal, null and range arguments without a GPU,
abnn_snapshot_diff_host against the numpy restatement (abnn_amd.snapshot) word
for word over every record-count edge, config and special weight pair, a
hand-made record array whose every header word is written out by hand, the four
invariants on every result, the merge of three slices, and the host rule in a
stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from snapshot_helpers import CONFIGS, N_NRN, NONE, SIZES, SPECIAL_PAIRS, SYN, UNEQUAL, invariants, pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
INF = float("inf")


def test_layouts_match_c(tmp_path):
    from abnn_amd import _lib

    cfg_fields = [n for n, _ in _lib.DiffConfig._fields_]
    info_fields = [n for n, _ in _lib.SnapshotInfo._fields_]
    consts = ["ABNN_SNAP_RECORDS", "ABNN_SNAP_STATE", "ABNN_DIFF_MAX_BINS", "ABNN_DIFF_HEADER_WORDS", "ABNN_ABI_VERSION"]
    prog = tmp_path / "sz.c"
    prog.write_text('#include "abnn/abnn.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                    'int main(void){printf("%zu %zu", sizeof(abnn_diff_config), sizeof(abnn_snapshot_info));\n'
                    + "".join(f'printf(" %u", (unsigned)({c}));\n' for c in consts)
                    + "".join(f'printf(" %zu", offsetof(abnn_diff_config, {f}));\n' for f in cfg_fields)
                    + "".join(f'printf(" %zu", offsetof(abnn_snapshot_info, {f}));\n' for f in info_fields)
                    + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(_lib.DiffConfig), C.sizeof(_lib.SnapshotInfo), _lib.SNAP_RECORDS, _lib.SNAP_STATE, _lib.DIFF_MAX_BINS,
            _lib.DIFF_HEADER_WORDS, _lib.ABI_VERSION, *(getattr(_lib.DiffConfig, f).offset for f in cfg_fields),
            *(getattr(_lib.SnapshotInfo, f).offset for f in info_fields)]
    assert got == want
    assert got[:7] == [32, 48, 1, 2, 4096, 24, 10]
    assert got[7:] == [0, 4, 8, 12, 16, 20, 24, 28, 0, 8, 16, 40]
    assert cfg_fields == ["lo", "hi", "bins", "src_first", "src_count", "dst_first", "dst_count", "reserved"]
    assert C.sizeof(_lib.DiffConfig) == C.sizeof(_lib.CensusConfig)  # the fields of abnn_census_config


def _invalid_configs():
    from abnn_amd import snapshot

    def tweak(cfg, **fields):
        for k, v in fields.items():
            setattr(cfg, k, v)
        return cfg

    return {
        "bins 0": snapshot.config(0, -1.0, 1.0),
        "bins 4097": snapshot.config(4097, -1.0, 1.0),
        "lo == hi": snapshot.config(8, 0.5, 0.5),
        "lo > hi": snapshot.config(8, 0.5, 0.25),
        "NaN lo": snapshot.config(8, np.nan, 1.0),
        "NaN hi": snapshot.config(8, 0.0, np.nan),
        "inf hi": snapshot.config(8, 0.0, INF),
        "-inf lo": snapshot.config(8, -INF, 0.0),
        "hi - lo overflows": snapshot.config(8, -3e38, 3e38),
        "bins / (hi - lo) overflows": snapshot.config(4096, 0.0, 1e-40),
        "reserved": tweak(snapshot.config(8, -1.0, 1.0), reserved=1),
    }


def test_diff_words():
    from abnn_amd import _lib, snapshot

    lib = _lib.load()
    for args in CONFIGS.values():
        cfg = snapshot.config(*args)
        assert lib.abnn_snapshot_diff_words(C.byref(cfg)) == 24 + cfg.bins == snapshot.n_words(cfg)
    for bins in (1, 2, 4095, 4096):
        cfg = snapshot.config(bins, -1e-3, 1e-3)
        assert lib.abnn_snapshot_diff_words(C.byref(cfg)) == 24 + bins == snapshot.n_words(cfg)
    empty = np.zeros(0, dtype=SYN)
    out = np.zeros(24 + 4097, dtype=np.uint64)
    for name, cfg in _invalid_configs().items():
        assert lib.abnn_snapshot_diff_words(C.byref(cfg)) == 0, name
        assert snapshot.n_words(cfg) == 0, name
        with pytest.raises(ValueError):
            snapshot.reference(empty, empty, cfg)
        assert lib.abnn_snapshot_diff_host(C.byref(cfg), N_NRN, None, 0, None, 0, out.ctypes.data) == 1, name
    assert lib.abnn_snapshot_diff_words(None) == 0
    cfg = snapshot.config(16, -0.5, 0.25, src=(1, 2), dst=(3, 4))
    assert (cfg.lo, cfg.hi, cfg.bins, cfg.src_first, cfg.src_count, cfg.dst_first, cfg.dst_count, cfg.reserved) == (
        -0.5, 0.25, 16, 1, 2, 3, 4, 0)


def test_null_and_range_arguments_are_invalid_without_a_gpu():
    from abnn_amd import _lib, snapshot

    lib = _lib.load()
    cfg = snapshot.config(8, -1.0, 1.0)
    rec = np.zeros(4, dtype=SYN)
    out = np.zeros(32, dtype=np.uint64)
    h = C.c_void_p()
    info = _lib.SnapshotInfo()
    assert lib.abnn_snapshot_create(None, C.byref(h)) == 1  # ABNN_ERR_INVALID
    assert lib.abnn_snapshot_create(None, None) == 1
    assert lib.abnn_snapshot_destroy(None) == 0
    assert lib.abnn_snapshot_get_info(None, C.byref(info)) == 1
    assert lib.abnn_snapshot_capture_enqueue(None, None, None) == 1
    assert lib.abnn_snapshot_restore(None, None, 3) == 1
    assert lib.abnn_snapshot_diff_enqueue(None, None, None, C.byref(cfg), out.ctypes.data, None) == 1
    assert lib.abnn_snapshot_diff(None, None, None, C.byref(cfg), out.ctypes.data, 32) == 1
    p = rec.ctypes.data
    assert lib.abnn_snapshot_diff_host(None, N_NRN, p, 4, p, 4, out.ctypes.data) == 1
    assert lib.abnn_snapshot_diff_host(C.byref(cfg), N_NRN, None, 4, p, 4, out.ctypes.data) == 1
    assert lib.abnn_snapshot_diff_host(C.byref(cfg), N_NRN, p, 4, None, 4, out.ctypes.data) == 1
    assert lib.abnn_snapshot_diff_host(C.byref(cfg), N_NRN, p, 4, p, 4, None) == 1
    for bad in (snapshot.config(8, -1.0, 1.0, dst=(990, 11)), snapshot.config(8, -1.0, 1.0, src=(1000, 1)),
                snapshot.config(8, -1.0, 1.0, src=(0xFFFFFFFF, 2))):
        assert lib.abnn_snapshot_diff_host(C.byref(bad), N_NRN, p, 4, p, 4, out.ctypes.data) == 1
    assert lib.abnn_snapshot_diff_host(C.byref(snapshot.config(8, -1.0, 1.0, dst=(990, 10))), N_NRN, p, 4, p, 4,
                                       out.ctypes.data) == 0
    assert lib.abnn_snapshot_diff_host(C.byref(cfg), N_NRN, None, 0, None, 0, out.ctypes.data) == 0 and not out.any()
    assert lib.abnn_snapshot_diff_host(C.byref(cfg), N_NRN, None, 0, p, 4, out.ctypes.data) == 0
    assert out[:5].tolist() == [4, 0, 0, 4, 0] and not out[5:].any()


def _host(cfg, then, now, n_nrn=N_NRN):
    from abnn_amd import _lib, snapshot

    then, now = np.ascontiguousarray(then), np.ascontiguousarray(now)
    out = np.full(24 + cfg.bins, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    st = _lib.load().abnn_snapshot_diff_host(C.byref(cfg), n_nrn, then.ctypes.data, len(then), now.ctypes.data,
                                             len(now), out.ctypes.data)
    assert st == 0, _lib.load().abnn_last_error()
    assert out[23] == 0
    d = snapshot.decode(out, cfg)
    assert snapshot.to_words(d).tolist() == out.tolist()
    invariants(d)
    return out


@pytest.mark.parametrize("sizes", [(n, n) for n in SIZES] + list(UNEQUAL))
def test_host_rule_equals_the_numpy_restatement(sizes):
    from abnn_amd import snapshot

    then, now = pair(*sizes, seed=sizes[0] + 1)
    c = min(sizes)
    for name, args in CONFIGS.items():
        cfg = snapshot.config(*args)
        want = snapshot.reference(then, now, cfg)
        invariants(want)
        got = _host(cfg, then, now)
        assert got.tolist() == snapshot.to_words(want).tolist(), (sizes, name)
        assert want["n_then"] == sizes[0] and want["n_now"] == sizes[1] and want["compared"] == c
    if c >= 4095:  # the cases reach what they are for
        d = snapshot.reference(then, now, snapshot.config(*CONFIGS["no range"]))
        for k in ("dead_both", "killed", "revived", "rewired", "same", "up", "down", "zero", "nan", "under", "over",
                  "not_summable"):
            assert d[k] > 0, k
        assert d["changed"] > c // 4 and np.isinf(d["max_abs"])
        narrow = snapshot.reference(then, now, snapshot.config(*CONFIGS["both"]))
        assert 0 < narrow["selected"] < d["selected"] and narrow["paired"] == d["paired"]


def test_special_pairs_one_by_one():
    """Every special pair alone, against what the rule says in words."""
    from abnn_amd import snapshot

    cfg = snapshot.config(4, -1.0, 1.0)
    want = {0: "nan", 1: "nan", 2: "zero", 3: "zero", 4: "same", 5: "down", 6: "up", 7: "down", 8: "up", 9: "down",
            10: "up", 11: "up", 12: "down", 13: "down", 14: "nan", 15: "up", 16: "up", 17: "down"}
    assert len(want) == len(SPECIAL_PAIRS)
    for j, (wa, wb) in enumerate(SPECIAL_PAIRS):
        then = np.array([(1, 2, wa, 0)], dtype=SYN)
        now = np.array([(1, 2, wb, 0)], dtype=SYN)
        d = snapshot.decode(_host(cfg, then, now), cfg)
        assert snapshot.to_words(snapshot.reference(then, now, cfg)).tolist() == snapshot.to_words(d).tolist(), j
        assert d[want[j]] == 1 and d["paired"] == d["selected"] == 1, (j, d)
        assert d["changed"] == (want[j] != "same")
    # the summable limit: 127.99999 is, 128 is not
    d = snapshot.decode(_host(cfg, np.array([(1, 2, 127.99999, 0)], dtype=SYN), np.array([(1, 2, -127.99999, 0)], dtype=SYN)), cfg)
    assert d["not_summable"] == 0 and d["net"] == -2 * (2**31 - 128) and d["abs"] == 2 * (2**31 - 128)
    d = snapshot.decode(_host(cfg, np.array([(1, 2, 127.99999, 0)], dtype=SYN), np.array([(1, 2, 128.0, 0)], dtype=SYN)), cfg)
    assert d["not_summable"] == 1 and d["net"] == 0 and d["abs"] == 0 and d["up"] == 1


def test_hand_made_records():
    """Twelve records against thirteen over ten neurons, four bins over
    [-1, 1) and dst in 5..8; every header word is written out by hand."""
    from abnn_amd import snapshot

    nan = np.nan
    then = np.array([(0, 5, 0.5, 0), (1, 5, 0.25, 0), (2, 6, 0.5, 0), (NONE, NONE, 0.75, 0), (3, 7, 1.0, 0),
                     (NONE, NONE, 0.0, 0), (0, 8, 0.5, 0), (9, 9, 0.125, 0), (5, 5, 0.0, 0), (1, 6, 2.0, 0),
                     (2, 6, nan, 0), (3, 8, 0.5, 0)], dtype=SYN)
    now = np.array([(0, 5, 0.75, 0),        # 0  changed, up by 0.25: bin 2, q +4194304
                    (1, 5, 0.25, 0),        # 1  same
                    (2, 6, 0.25, 0),        # 2  changed, down by 0.25: bin 1, q -4194304
                    (NONE, NONE, 0.1, 0),   # 3  dead on both sides
                    (NONE, NONE, 1.0, 0),   # 4  killed
                    (4, 7, 0.5, 0),         # 5  revived
                    (0, 7, 0.5, 0),         # 6  rewired
                    (9, 9, 0.5, 0),         # 7  paired, dst 9 is outside the range
                    (5, 5, -0.0, 0),        # 8  changed, zero: d = -0.0 falls into bin 2, q 0
                    (1, 6, -1.0, 0),        # 9  changed, down by 3: under, q -50331648
                    (2, 6, 0.5, 0),         # 10 changed, nan: not summable
                    (3, 8, 200.0, 0),       # 11 changed, up by 199.5: over, not summable
                    (4, 5, 0.5, 0)],        # 12 born
                   dtype=SYN)
    cfg = snapshot.config(4, -1.0, 1.0, dst=(5, 4))
    got = _host(cfg, then, now, n_nrn=10)
    net = 4194304 - 4194304 + 0 - 50331648
    head = [13, 12, 12, 1, 0,            # n_now n_then compared born gone
            1, 1, 1, 1, 8,               # dead_both killed revived rewired paired
            7, 1, 6, 2, 2, 1, 1,         # selected same changed up down zero nan
            1, 1,                        # under over
            net + 2**64, 4194304 + 4194304 + 50331648, 2,   # net abs not_summable
            0x43478000, 0]               # the bits of 199.5
    assert got[:24].tolist() == head and got[24:].tolist() == [0, 1, 2, 0]
    assert snapshot.to_words(snapshot.reference(then, now, cfg)).tolist() == got.tolist()
    d = snapshot.decode(got, cfg)
    assert d["net"] == net and d["max_abs"] == F32(199.5)
    # the other way round: born and gone, killed and revived, up and down change places
    back = snapshot.decode(_host(cfg, now, then, n_nrn=10), cfg)
    assert (back["born"], back["gone"], back["killed"], back["revived"], back["up"], back["down"]) == (0, 1, 1, 1, 2, 2)
    assert back["net"] == -net and back["abs"] == d["abs"] and back["counts"].tolist() == [0, 1, 2, 0] and back["over"] == 1


@pytest.mark.parametrize("sizes", [(8193, 8193), (4099, 4096), (4097, 4099)])
def test_merge_of_three_slices_equals_the_whole(sizes):
    from abnn_amd import snapshot

    then, now = pair(*sizes, seed=5)
    for args in CONFIGS.values():
        cfg = snapshot.config(*args)
        whole = snapshot.reference(then, now, cfg)
        parts = [snapshot.decode(_host(cfg, then[lo:hi], now[lo:hi]), cfg) for lo, hi in ((0, 3000), (3000, 4096), (4096, 10_000))]
        merged = snapshot.merge(parts)
        invariants(merged)
        assert snapshot.to_words(merged).tolist() == snapshot.to_words(whole).tolist()
    with pytest.raises(ValueError):
        snapshot.merge([])


def test_host_rule_under_the_sanitizers(tmp_path):
    """csrc/snapshot.h's host rule in a stand-alone program built with
    -fsanitize=address,undefined, run once over every size pair and config."""
    from abnn_amd import snapshot
    from abnn_amd.build import build_snapshot_host_test

    prog = build_snapshot_host_test(out=str(tmp_path / "snapshot_host_test"))
    cases = []
    for sizes in [(n, n) for n in SIZES] + list(UNEQUAL) + [(0, 5), (5, 0)]:
        then, now = pair(*sizes, seed=sizes[1] + 3)
        cases += [(snapshot.config(*args), then, now) for args in CONFIGS.values()]
    blob = [struct.pack("<Q", len(cases))]
    for cfg, then, now in cases:
        blob += [bytes(cfg), struct.pack("<2Q", len(then), len(now)), then.tobytes(), now.tobytes()]
    (tmp_path / "in.bin").write_bytes(b"".join(blob))
    r = subprocess.run([prog, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    out = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.uint64)
    at = 0
    for cfg, then, now in cases:
        words = 24 + cfg.bins
        assert out[at:at + words].tolist() == snapshot.to_words(snapshot.reference(then, now, cfg)).tolist(), bytes(cfg).hex()
        at += words
    assert at == len(out)
