"""The record reorder (abnn.h ``abnn_reorder_*``) on the host side.

The reorder itself runs in the HIP library (csrc/reorder.hip, the rule in
csrc/reorder.h); this module holds what needs no GPU: the config, the 32-bit
keys, the numpy restatement of the rule over interchange records
(:func:`reference`: the test reference, and usable for small brains), the
decoding of a result and the inverse of a returned ``origin``.  The key is
integer arithmetic and the order is a stable sort, so :func:`reference` equals
the device and ``abnn_reorder_host`` word for word.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple, Union

import numpy as np

from ._lib import (REORDER_DESCENDING, REORDER_DST, REORDER_HEADER_WORDS, REORDER_KEY, REORDER_NONE, REORDER_ORIGIN,
                   REORDER_PERM, REORDER_RANDOM, REORDER_SRC, REORDER_W, ReorderConfig)
from .graph import _splitmix64_at

U32 = np.uint32
U64 = np.uint64
# csrc/reorder.h kReorderTile: the records (keys pass) or (key, index) pairs
# (radix passes) one workgroup loads at a time
TILE = 4096
# the interchange record (brain.SYN_DTYPE)
SYN_DTYPE = np.dtype([("src", "<u4"), ("dst", "<u4"), ("w", "<f4"), ("pad", "<f4")])
KEYS = {"src": REORDER_SRC, "dst": REORDER_DST, "w": REORDER_W, "random": REORDER_RANDOM, "none": REORDER_NONE,
        "perm": REORDER_PERM}
HEADER_KEYS = ("records", "tombstones", "moved", "invalid", "syn_offset")  # words 0..4
MAX_RECORDS = 1 << 32  # local indices are u32
_ALL = REORDER_DESCENDING | REORDER_ORIGIN
_TOMB = U32(0xFFFFFFFF)


def key_code(key: Union[int, str]) -> int:
    if isinstance(key, str):
        if key not in KEYS:
            raise ValueError(f"reorder: unknown key {key!r} (one of {sorted(KEYS)})")
        return KEYS[key]
    return int(key)


def config(key: Union[int, str], descending: bool = False, seed: int = 0, origin: bool = False) -> ReorderConfig:
    """``key``: 'src', 'dst', 'w', 'random', 'none' or 'perm' (or its code);
    ``descending`` for src, dst and w; ``seed`` for random; ``origin``: the
    result also holds the permutation."""
    flags = (REORDER_DESCENDING if descending else 0) | (REORDER_ORIGIN if origin else 0)
    return ReorderConfig(key_code(key), flags, int(seed) & (2**64 - 1), (C.c_uint32 * 4)())


def config_ok(cfg: Optional[ReorderConfig]) -> bool:
    """The checks of abnn_reorder_words that need no record count."""
    if cfg is None or cfg.key > REORDER_PERM or cfg.flags & ~_ALL or any(cfg.reserved):
        return False
    if cfg.flags & REORDER_DESCENDING and cfg.key > REORDER_W:
        return False
    if cfg.key != REORDER_RANDOM and cfg.seed:
        return False
    return True


def n_words(cfg: Optional[ReorderConfig], n_syn: int) -> int:
    """abnn_reorder_words: 8 + (ORIGIN ? (n_syn + 1) // 2 : 0), or 0 for an
    invalid config or more than 2**32 records."""
    n_syn = int(n_syn)
    if not config_ok(cfg) or n_syn < 0 or n_syn > MAX_RECORDS:
        return 0
    return REORDER_HEADER_WORDS + ((n_syn + 1) // 2 if cfg.flags & REORDER_ORIGIN else 0)


def keys(syn: np.ndarray, cfg: ReorderConfig, syn_offset: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """(tomb, k32) of abnn.h for every record: the tombstone bit (bool) and the
    32-bit key (np.uint32; 0 for a tombstone, inverted with DESCENDING)."""
    n = len(syn)
    dst = syn["dst"].astype(U32)
    tomb = dst == _TOMB
    if cfg.key == REORDER_SRC:
        k = syn["src"].astype(U32)
    elif cfg.key == REORDER_DST:
        k = dst.copy()
    elif cfg.key == REORDER_W:
        b = np.ascontiguousarray(syn["w"], dtype=np.float32).view(U32)
        k = b ^ np.where(b >> U32(31), U32(0xFFFFFFFF), U32(0x80000000)).astype(U32)
    elif cfg.key == REORDER_RANDOM:
        at = np.arange(n, dtype=U64) + U64(syn_offset)
        k = (_splitmix64_at((int(cfg.seed) ^ REORDER_KEY) & (2**64 - 1), at) >> U64(32)).astype(U32)
    else:
        k = np.zeros(n, dtype=U32)
    if cfg.flags & REORDER_DESCENDING:
        k = ~k
    k = k.astype(U32)
    k[tomb] = 0
    return tomb, k


def reference(syn: np.ndarray, cfg: ReorderConfig, syn_offset: int = 0,
              perm: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray, dict]:
    """The reorder of interchange records ``syn`` in numpy: (records, origin,
    header) -- the reordered records (SYN_DTYPE, pad 0), the permutation
    (np.uint32; the identity after an invalid perm) and the header counts
    (HEADER_KEYS)."""
    n = len(syn)
    if not n_words(cfg, n) or (cfg.key == REORDER_PERM) != (perm is not None):
        raise ValueError("reorder: invalid config")
    tomb, k32 = keys(syn, cfg, syn_offset)
    invalid = 0
    if cfg.key == REORDER_PERM:
        p = np.ascontiguousarray(perm, dtype=U32)
        if p.shape != (n,):
            raise ValueError("reorder: perm must hold n_syn entries")
        inside = p[p < n]
        invalid = int(n - len(inside)) + int(len(inside) - len(np.unique(inside)))
        origin = p.copy() if invalid == 0 else np.arange(n, dtype=U32)
    else:
        origin = np.lexsort((k32, tomb)).astype(U32)  # stable; the last key is the primary one
    rec = np.zeros(n, dtype=SYN_DTYPE)
    for f in ("src", "dst"):
        rec[f] = syn[f][origin]
    rec["w"].view(U32)[:] = np.ascontiguousarray(syn["w"], dtype=np.float32).view(U32)[origin]
    header = {"records": n, "tombstones": int(tomb.sum()), "moved": int((origin != np.arange(n, dtype=U32)).sum()),
              "invalid": invalid, "syn_offset": int(syn_offset)}
    return rec, origin, header


def inverse(origin: np.ndarray) -> np.ndarray:
    """The permutation that undoes ``origin``: reorder(perm=inverse(origin))
    after a reorder that returned ``origin`` gives the first order back."""
    origin = np.ascontiguousarray(origin, dtype=U32)
    inv = np.empty(len(origin), dtype=U32)
    inv[origin] = np.arange(len(origin), dtype=U32)
    return inv


def decode(words: np.ndarray, cfg: ReorderConfig) -> dict:
    """A result's u64 words (abnn.h) as a dict: the header counts and, with
    ORIGIN, ``origin`` (np.uint32, one entry per record)."""
    w = np.ascontiguousarray(words, dtype=U64)
    d = {k: int(w[i]) for i, k in enumerate(HEADER_KEYS)}
    n = d["records"]
    assert w.shape == (n_words(cfg, n),), (w.shape, n)
    if cfg.flags & REORDER_ORIGIN:
        d["origin"] = w[REORDER_HEADER_WORDS:].view(U32)[:n].copy()
    return d


def to_words(header: dict, cfg: ReorderConfig, origin: Optional[np.ndarray] = None) -> np.ndarray:
    """The inverse of :func:`decode`: the result's u64 words."""
    n = int(header["records"])
    w = np.zeros(n_words(cfg, n), dtype=U64)
    w[:5] = [header[k] for k in HEADER_KEYS]
    if cfg.flags & REORDER_ORIGIN:
        w[REORDER_HEADER_WORDS:].view(U32)[:n] = np.ascontiguousarray(origin, dtype=U32)
    return w
