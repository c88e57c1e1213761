"""CPU checks of the record reorder's boundary (abnn.h abnn_reorder_*): the
ctypes mirror matches the C layout and the constants, every refusal of
abnn_reorder_words, null handles without a GPU, abnn_reorder_host against the
numpy restatement (abnn_amd.reorder.reference) word for word -- every key in
both directions, PERM valid and invalid, syn_offset != 0, n in {0, 1, 2, 3}, the
special weights -- a hand-made array whose result is written out by hand, and
the host rule in a stand-alone program under the sanitizers."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U32 = np.uint32
NONE = 0xFFFFFFFF
SYN = [("src", "<u4"), ("dst", "<u4"), ("w", "<f4"), ("pad", "<f4")]
SPECIAL_BITS = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000,
                         0x00012345, 0x80012345], dtype=U32)  # NaN (+, -, signalling), +-inf, -0.0, +0.0, denormals


def test_reorder_config_layout_matches_c(tmp_path):
    from abnn_amd import _lib

    names = ["ABNN_REORDER_SRC", "ABNN_REORDER_DST", "ABNN_REORDER_W", "ABNN_REORDER_RANDOM", "ABNN_REORDER_NONE",
             "ABNN_REORDER_PERM", "ABNN_REORDER_DESCENDING", "ABNN_REORDER_ORIGIN", "ABNN_REORDER_HEADER_WORDS",
             "ABNN_REORDER_SCRATCH_BYTES_PER_RECORD"]
    prog = tmp_path / "sz.c"
    prog.write_text('#include "abnn/abnn.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                    'int main(void){printf("%zu %llu", sizeof(abnn_reorder_config), (unsigned long long)ABNN_REORDER_KEY);\n'
                    + "".join(f'printf(" %u", (unsigned)({n}));\n' for n in names)
                    + "".join(f'printf(" %zu", offsetof(abnn_reorder_config, {f}));\n' for f in ("key", "flags", "seed", "reserved"))
                    + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(_lib.ReorderConfig), _lib.REORDER_KEY,
            *(getattr(_lib, n[len("ABNN_"):]) for n in names),
            *(getattr(_lib.ReorderConfig, f).offset for f in ("key", "flags", "seed", "reserved"))]
    assert got == want
    assert got[0] == 32 and got[1] == 0xC2B2AE3D27D4EB4F
    assert got[2:12] == [0, 1, 2, 3, 4, 5, 1, 2, 8, 28]
    assert got[12:] == [0, 4, 8, 16]
    assert [n for n, _ in _lib.ReorderConfig._fields_] == ["key", "flags", "seed", "reserved"]
    assert _lib.load().abnn_abi_version() == 10  # the entry points are additions


def test_tile_mirrors_the_header():
    from abnn_amd import reorder

    with open(os.path.join(ROOT, "abnn_amd", "csrc", "reorder.h")) as f:
        text = f.read()
    m = re.search(r"kReorderTile\s*=\s*(\d+)\s*;", text)
    assert m and int(m.group(1)) == reorder.TILE
    assert reorder.SYN_DTYPE == np.dtype(SYN)


def _edit(cfg, **kw):
    for k, v in kw.items():
        if k.startswith("reserved"):
            cfg.reserved[int(k[-1])] = v
        else:
            setattr(cfg, k, v)
    return cfg


def _invalid_configs():
    """name -> config: every refusal abnn.h lists that needs no handle (null is checked apart)."""
    from abnn_amd import reorder

    return {
        "key 6": _edit(reorder.config("src"), key=6),
        "key 2^31": _edit(reorder.config("src"), key=1 << 31),
        "flag bit 2": _edit(reorder.config("dst"), flags=4),
        "flag bit 31 with valid bits": _edit(reorder.config("dst", origin=True), flags=2 | 1 << 31),
        "reserved[0]": _edit(reorder.config("w"), reserved0=1),
        "reserved[3]": _edit(reorder.config("w"), reserved3=1 << 31),
        "seed with src": _edit(reorder.config("src"), seed=1),
        "seed with none": _edit(reorder.config("none"), seed=1 << 63),
        "seed with perm": _edit(reorder.config("perm"), seed=5),
        "descending none": reorder.config("none", descending=True),
        "descending random": reorder.config("random", descending=True, seed=3),
        "descending perm": reorder.config("perm", descending=True),
    }


def _valid_configs():
    from abnn_amd import reorder

    return {
        "src": reorder.config("src"), "dst descending": reorder.config("dst", descending=True),
        "w with origin": reorder.config("w", origin=True), "w descending, origin": reorder.config("w", True, 0, True),
        "random": reorder.config("random", seed=(1 << 64) - 1), "random, seed 0": reorder.config("random"),
        "none": reorder.config("none", origin=True), "perm": reorder.config("perm"), "perm, origin": reorder.config("perm", origin=True),
    }


def test_reorder_words():
    from abnn_amd import _lib, reorder

    lib = _lib.load()
    empty = np.zeros(0, dtype=SYN)
    for name, cfg in _valid_configs().items():
        for n in (0, 1, 2, 3, 4097, (1 << 32) - 1, 1 << 32):
            want = 8 + ((n + 1) // 2 if cfg.flags & _lib.REORDER_ORIGIN else 0)
            assert lib.abnn_reorder_words(C.byref(cfg), n) == want == reorder.n_words(cfg, n), (name, n)
        for n in ((1 << 32) + 1, 1 << 40, (1 << 64) - 1):  # local indices are u32
            assert lib.abnn_reorder_words(C.byref(cfg), n) == 0 == reorder.n_words(cfg, n), (name, n)
    for name, cfg in _invalid_configs().items():
        for n in (0, 5):
            assert lib.abnn_reorder_words(C.byref(cfg), n) == 0, name
            assert reorder.n_words(cfg, n) == 0, name
        out = (C.c_uint64 * 8)()
        assert lib.abnn_reorder_host(C.byref(cfg), 0, None, 0, None, out) == 1, name
        with pytest.raises(ValueError):
            reorder.reference(empty, cfg, perm=empty["src"] if cfg.key == _lib.REORDER_PERM else None)
    assert lib.abnn_reorder_words(None, 4) == 0 and reorder.n_words(None, 4) == 0
    # config(): the flags follow the arguments; names and codes
    c = reorder.config("w", descending=True, origin=True)
    assert (c.key, c.flags, c.seed, list(c.reserved)) == (2, 3, 0, [0, 0, 0, 0])
    assert reorder.config(3, seed=77).seed == 77 and reorder.config("random", seed=-1).seed == (1 << 64) - 1
    with pytest.raises(ValueError):
        reorder.config("weight")


def test_reorder_null_arguments_are_invalid_without_a_gpu():
    from abnn_amd import _lib, reorder

    lib = _lib.load()
    cfg = reorder.config("dst")
    out = (C.c_uint64 * 8)()
    rec = np.zeros(2, dtype=SYN)
    perm = np.arange(2, dtype=U32)
    assert lib.abnn_reorder_enqueue(None, C.byref(cfg), None, out, None) == 1  # ABNN_ERR_INVALID
    assert lib.abnn_reorder(None, C.byref(cfg), None, out, 8) == 1
    assert lib.abnn_reorder(None, None, None, None, 0) == 1
    assert lib.abnn_reorder_release(None) == 1
    assert lib.abnn_reorder_host(None, 0, rec.ctypes.data, 2, None, out) == 1
    assert lib.abnn_reorder_host(C.byref(cfg), 0, None, 2, None, out) == 1
    assert lib.abnn_reorder_host(C.byref(cfg), 0, rec.ctypes.data, 2, None, None) == 1
    assert lib.abnn_reorder_host(C.byref(cfg), 0, rec.ctypes.data, 2, perm.ctypes.data, out) == 1  # a perm without PERM
    assert lib.abnn_reorder_host(C.byref(reorder.config("perm")), 0, rec.ctypes.data, 2, None, out) == 1  # PERM without one
    assert lib.abnn_reorder_host(C.byref(cfg), 0, rec.ctypes.data, 2, None, out) == 0


def _records(n, seed, n_nrn=50):
    """Seeded records over few neurons (long runs of equal keys), a tenth of them
    tombstones, the special weights at the first, a middle and the last index."""
    rng = np.random.default_rng(seed)
    syn = np.zeros(n, dtype=SYN)
    syn["src"] = rng.integers(0, n_nrn, n, dtype=U32)
    syn["dst"] = rng.integers(0, n_nrn, n, dtype=U32)
    syn["w"] = rng.uniform(-0.1, 1.1, n).astype(F32)
    syn["pad"] = 7.0  # never carried over
    k = len(SPECIAL_BITS)
    if n >= 3 * k:
        for at in (0, n // 2 - k // 2, n - k):
            syn["w"].view(U32)[at:at + k] = SPECIAL_BITS
    else:
        for j, at in enumerate(sorted({0, n // 2, n - 1} & set(range(n)))):
            syn["w"].view(U32)[at] = SPECIAL_BITS[(seed + j) % k]
    dead = rng.random(n) < 0.1
    syn["src"][dead] = syn["dst"][dead] = NONE
    return syn


def _cases(n, seed):
    """(config, perm) over n records: every key in both directions, with and
    without the origin plane, two seeds, PERM valid and invalid."""
    from abnn_amd import reorder

    rng = np.random.default_rng(seed + 100)
    cases = []
    for key in ("src", "dst", "w"):
        for desc in (False, True):
            cases.append((reorder.config(key, desc, origin=True), None))
    cases += [(reorder.config("w"), None), (reorder.config("none", origin=True), None), (reorder.config("none"), None),
              (reorder.config("random", seed=1, origin=True), None), (reorder.config("random", seed=0xDEADBEEFCAFEF00D, origin=True), None)]
    good = rng.permutation(n).astype(U32)
    cases += [(reorder.config("perm", origin=True), good), (reorder.config("perm"), np.arange(n, dtype=U32))]
    if n >= 1:
        cases.append((reorder.config("perm", origin=True), np.full(n, n, dtype=U32)))  # every entry equal to n
    if n >= 2:
        rep = good.copy()
        rep[-1] = rep[0]
        cases.append((reorder.config("perm", origin=True), rep))  # one repeat
        far = good.copy()
        far[n // 2] = NONE
        far[0] = far[1]
        cases.append((reorder.config("perm"), far))  # one out of range and one repeat
    return cases


def _host(cfg, syn, offset, perm):
    from abnn_amd import _lib

    lib = _lib.load()
    n = len(syn)
    words = lib.abnn_reorder_words(C.byref(cfg), n)
    out = np.full(words, 0xABABABABABABABAB, dtype=np.uint64)
    rec = syn.copy()
    p = None if perm is None else np.ascontiguousarray(perm, dtype=U32)
    # PERM over no record: any non-null pointer
    ptr = None if p is None else (p.ctypes.data if n else out.ctypes.data)
    assert lib.abnn_reorder_host(C.byref(cfg), offset, rec.ctypes.data if n else None, n, ptr, out.ctypes.data) == 0
    return rec, out


@pytest.mark.parametrize("n", [0, 1, 2, 3, 64, 65, 1000, 4097])
def test_host_rule_equals_the_numpy_restatement(n):
    from abnn_amd import reorder

    syn = _records(n, n + 3)
    for offset in (0, 12345, (1 << 40) + 7):
        for cfg, perm in _cases(n, n):
            rec, out = _host(cfg, syn, offset, perm)
            want, origin, head = reorder.reference(syn, cfg, offset, perm)
            assert np.array_equal(out, reorder.to_words(head, cfg, origin)), (n, offset, bytes(cfg).hex())
            assert np.array_equal(rec.view(U32), want.view(U32)), (n, offset, bytes(cfg).hex())
            assert not rec["pad"].any() and head["records"] == n and head["syn_offset"] == offset
            got = reorder.decode(out, cfg)
            assert {k: got[k] for k in reorder.HEADER_KEYS} == head
            if cfg.key != 5:  # the tombstones are exactly the last ones, in their old order
                t = head["tombstones"]
                assert (want["dst"][n - t:] == NONE).all() and (want["dst"][:n - t] != NONE).all()
                if "origin" in got:
                    assert (np.diff(got["origin"][n - t:].astype(np.int64)) > 0).all()
            elif head["invalid"]:
                assert head["moved"] == 0 and np.array_equal(rec.view(U32).reshape(-1, 4)[:, :3], syn.view(U32).reshape(-1, 4)[:, :3])


def test_hand_made_records():
    """Eight records; the expected orders are written out by hand."""
    from abnn_amd import reorder

    w = np.array([0.5, -0.0, 9.0, 0.0, np.nan, -1.0, np.inf, 0.5], dtype=F32)
    w.view(U32)[4] = 0xFFC00000  # a negative NaN: below -inf in the key's order
    src = [3, 1, NONE, 1, 2, 0, 3, 1]
    dst = [4, 5, NONE, 5, 4, 6, 4, NONE]  # records 2 and 7 are tombstones
    syn = np.zeros(8, dtype=SYN)
    syn["src"], syn["dst"], syn["w"] = src, dst, w
    want = {
        ("src", False): [5, 1, 3, 4, 0, 6, 2, 7],
        ("src", True): [0, 6, 4, 1, 3, 5, 2, 7],
        ("dst", False): [0, 4, 6, 1, 3, 5, 2, 7],
        ("dst", True): [5, 1, 3, 0, 4, 6, 2, 7],
        ("w", False): [4, 5, 1, 3, 0, 6, 2, 7],   # -NaN < -1 < -0.0 < +0.0 < 0.5 < +inf, then the tombstones
        ("w", True): [6, 0, 3, 1, 5, 4, 2, 7],
        ("none", False): [0, 1, 3, 4, 5, 6, 2, 7],
    }
    for (key, desc), origin in want.items():
        cfg = reorder.config(key, desc, origin=True)
        rec, got, head = reorder.reference(syn, cfg, 9)
        assert got.tolist() == origin, (key, desc)
        assert head == {"records": 8, "tombstones": 2, "moved": sum(o != k for k, o in enumerate(origin)), "invalid": 0,
                        "syn_offset": 9}
        assert np.array_equal(rec.view(U32), syn[origin].view(U32))
        hrec, out = _host(cfg, syn, 9, None)
        assert np.array_equal(out, reorder.to_words(head, cfg, got)) and np.array_equal(hrec.view(U32), rec.view(U32))
        # undone by the inverse
        back, _, h2 = reorder.reference(rec, reorder.config("perm"), 9, reorder.inverse(got))
        assert np.array_equal(back.view(U32), syn.view(U32)) and h2["moved"] == head["moved"]
    assert reorder.to_words({"records": 3, "tombstones": 0, "moved": 2, "invalid": 0, "syn_offset": 1},
                            reorder.config("src", origin=True), [2, 1, 0]).tolist() == [3, 0, 2, 0, 1, 0, 0, 0, 2 | 1 << 32, 0]


def test_random_keys_spread_over_shards():
    """A shard draws what the unsharded brain draws for the same global index."""
    from abnn_amd import reorder

    n = 10_000
    syn = _records(n, 2)
    cfg = reorder.config("random", seed=42)
    _, whole = reorder.keys(syn, cfg, 0)
    for lo, hi in ((0, 3_334), (3_334, 6_667), (6_667, n)):
        _, part = reorder.keys(syn[lo:hi], cfg, lo)
        assert np.array_equal(part, whole[lo:hi])
    live = syn["dst"] != NONE
    assert len(np.unique(whole[live])) > 0.99 * live.sum() and not whole[~live].any()
    _, other = reorder.keys(syn, reorder.config("random", seed=43), 0)
    assert (other[live] != whole[live]).mean() > 0.99


def test_host_rule_under_the_sanitizers(tmp_path):
    """csrc/reorder.h's host rule in a stand-alone program built with
    -fsanitize=address,undefined, run once over small arrays of every key."""
    from abnn_amd import reorder
    from abnn_amd.build import build_reorder_host_test

    prog = build_reorder_host_test(out=str(tmp_path / "reorder_host_test"))
    cases = []
    for n in (0, 1, 2, 3, 65, 1000):
        syn = _records(n, n + 1)
        cases += [(cfg, perm, syn, 123 if cfg.key == 3 else 0) for cfg, perm in _cases(n, n)]
    blob = [struct.pack("<Q", len(cases))]
    for cfg, perm, syn, offset in cases:
        m = 0 if perm is None else len(perm)
        blob += [bytes(cfg), struct.pack("<3Q", offset, len(syn), m), syn.tobytes(), b"" if perm is None else perm.tobytes()]
    (tmp_path / "in.bin").write_bytes(b"".join(blob))
    r = subprocess.run([prog, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    out = (tmp_path / "out.bin").read_bytes()
    at = 0
    for cfg, perm, syn, offset in cases:
        want, origin, head = reorder.reference(syn, cfg, offset, perm)
        words = reorder.n_words(cfg, len(syn))
        got = np.frombuffer(out, dtype=np.uint64, count=words, offset=at)
        at += 8 * words
        assert np.array_equal(got, reorder.to_words(head, cfg, origin)), bytes(cfg).hex()
        assert out[at:at + 16 * len(syn)] == want.tobytes(), bytes(cfg).hex()
        at += 16 * len(syn)
    assert at == len(out)
