"""The synapse select (abnn.h ``abnn_select_*``) on the host side.

The select itself runs in the HIP library (csrc/select.hip); this module holds
what needs no GPU: the config, the decoding of a result into a dict, the numpy
restatement of the matching rule over interchange records (:func:`reference`:
the test reference, and usable for small brains) and the merge of the shards'
results (:func:`merge`).  Every comparison of the rule is one uint32 or float32
operation and the output order is the record order, so :func:`reference` equals
the device bit for bit.
"""
from __future__ import annotations

from typing import Iterable, Optional, Sequence

import numpy as np

from ._lib import SELECT_ANY, SELECT_HEADER_WORDS, SELECT_WEIGHT, SelectConfig

F32 = np.float32
U32 = np.uint32
# csrc/select.h kSelectTile: the consecutive records one workgroup loads at a
# time; the count launch leaves one match count per tile, the emit launch skips
# the tiles without a match
TILE = 4096
# the interchange record (brain.SYN_DTYPE)
SYN_DTYPE = np.dtype([("src", "<u4"), ("dst", "<u4"), ("w", "<f4"), ("pad", "<f4")])
_COUNT_KEYS = ("records", "tombstones", "matched", "written", "syn_offset")  # words 0..4
_ALL = SELECT_ANY | SELECT_WEIGHT


def config(src: Optional[Sequence[int]] = None, dst: Optional[Sequence[int]] = None,
           weights: Optional[Sequence[float]] = None, any: bool = False) -> SelectConfig:
    """``src`` / ``dst`` are (first, count) neuron ranges, None = not set;
    ``weights`` = (w_lo, w_hi) keeps w_lo <= w < w_hi (inf allowed); ``any``:
    a record matches when either set range holds, not both."""
    sf, sc = (0, 0) if src is None else (int(src[0]), int(src[1]))
    df, dc = (0, 0) if dst is None else (int(dst[0]), int(dst[1]))
    lo, hi = (0.0, 0.0) if weights is None else (float(weights[0]), float(weights[1]))
    flags = (SELECT_ANY if any else 0) | (SELECT_WEIGHT if weights is not None else 0)
    return SelectConfig(sf, sc, df, dc, lo, hi, flags, 0)


def _bits(x: float) -> int:
    return int(np.array([x], dtype=F32).view(U32)[0])


def config_ok(cfg: Optional[SelectConfig], n_nrn: Optional[int] = None) -> bool:
    """The checks of abnn_select_words; with ``n_nrn`` also the handle's (a set
    range ends at or below N_NRN)."""
    if cfg is None or cfg.flags & ~_ALL or cfg.reserved:
        return False
    if cfg.src_first + cfg.src_count > 1 << 32 or cfg.dst_first + cfg.dst_count > 1 << 32:
        return False
    if cfg.flags & SELECT_ANY and not (cfg.src_count or cfg.dst_count):
        return False
    if cfg.flags & SELECT_WEIGHT:
        if not F32(cfg.w_lo) < F32(cfg.w_hi):  # false for a NaN bound
            return False
    elif _bits(cfg.w_lo) or _bits(cfg.w_hi):
        return False
    if n_nrn is not None:
        if cfg.src_count and cfg.src_first + cfg.src_count > int(n_nrn):
            return False
        if cfg.dst_count and cfg.dst_first + cfg.dst_count > int(n_nrn):
            return False
    return True


def n_words(cfg: SelectConfig, capacity: int) -> int:
    """abnn_select_words: 8 + 3 * capacity, or 0 for an invalid config."""
    capacity = int(capacity)
    if not config_ok(cfg) or capacity < 0 or capacity > ((1 << 64) - 1 - SELECT_HEADER_WORDS) // 3:
        return 0
    return SELECT_HEADER_WORDS + 3 * capacity


def matches(syn: np.ndarray, cfg: SelectConfig) -> np.ndarray:
    """The matching rule of abnn.h over interchange records: a bool per record."""
    src, dst = syn["src"].astype(U32), syn["dst"].astype(U32)
    m = dst != U32(0xFFFFFFFF)
    s = (src - U32(cfg.src_first)) < U32(cfg.src_count)  # uint32 arithmetic: wraps
    d = (dst - U32(cfg.dst_first)) < U32(cfg.dst_count)
    if cfg.flags & SELECT_ANY:
        m &= s | d  # a range that is not set has count 0: false
    else:
        if cfg.src_count:
            m &= s
        if cfg.dst_count:
            m &= d
    if cfg.flags & SELECT_WEIGHT:
        w = syn["w"].astype(F32)
        with np.errstate(invalid="ignore"):
            m &= (w >= F32(cfg.w_lo)) & (w < F32(cfg.w_hi))  # false for NaN
    return m


def reference(syn: np.ndarray, cfg: SelectConfig, capacity: int, n_nrn: int, syn_offset: int = 0) -> dict:
    """The select of interchange records ``syn`` (fields src, dst, w) in numpy:
    records, tombstones, matched, written, syn_offset, capacity, ``index``
    (np.uint64, global) and ``syn`` (SYN_DTYPE, pad 0), both trimmed to written."""
    capacity = int(capacity)
    if not config_ok(cfg, n_nrn) or not n_words(cfg, capacity):
        raise ValueError("select: invalid config")
    at = np.flatnonzero(matches(syn, cfg))
    written = min(len(at), capacity)
    rec = np.zeros(written, dtype=SYN_DTYPE)
    for f in ("src", "dst", "w"):
        rec[f] = syn[f][at[:written]]
    return {"records": int(len(syn)), "tombstones": int((syn["dst"].astype(U32) == U32(0xFFFFFFFF)).sum()),
            "matched": int(len(at)), "written": written, "syn_offset": int(syn_offset), "capacity": capacity,
            "index": at[:written].astype(np.uint64) + np.uint64(syn_offset), "syn": rec}


def decode(words: np.ndarray, capacity: int) -> dict:
    """A result's u64 words (abnn.h) as a dict: the header counts, capacity,
    ``index`` (np.uint64) and ``syn`` (SYN_DTYPE), both trimmed to written."""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    capacity = int(capacity)
    h = SELECT_HEADER_WORDS
    assert w.shape == (h + 3 * capacity,), (w.shape, capacity)
    d = {k: int(w[i]) for i, k in enumerate(_COUNT_KEYS)}
    n = d["written"]
    assert n <= capacity and n <= d["matched"], d
    d["capacity"] = capacity
    d["index"] = w[h:h + n].copy()
    d["syn"] = w[h + capacity:h + capacity + 2 * n].view(SYN_DTYPE).copy()
    return d


def to_words(d: dict) -> np.ndarray:
    """The inverse of :func:`decode`: the result's u64 words, the plane entries
    at and past written (which the device does not write) as zeros."""
    h, cap, n = SELECT_HEADER_WORDS, int(d["capacity"]), int(d["written"])
    w = np.zeros(h + 3 * cap, dtype=np.uint64)
    w[:5] = [d[k] for k in _COUNT_KEYS]
    w[h:h + n] = d["index"]
    w[h + cap:h + cap + 2 * n] = np.ascontiguousarray(d["syn"], dtype=SYN_DTYPE).view(np.uint64)
    return w


def merge(parts: Iterable[dict], capacity: int) -> dict:
    """The select of the concatenation of the shards' records from their
    results under one config, ``parts`` in rank order: the indices are already
    global, so the planes concatenate and are cut to the first ``capacity``;
    records, tombstones and matched add.  Every part must have been selected
    with a capacity that leaves it the entries the merged result needs
    (``capacity`` itself always does)."""
    parts = list(parts)
    capacity = int(capacity)
    if not parts:
        raise ValueError("merge: no results")
    out = {k: sum(int(p[k]) for p in parts) for k in ("records", "tombstones", "matched")}
    need = capacity
    for p in parts:
        if int(p["written"]) < min(int(p["matched"]), need):
            raise ValueError("merge: a part holds fewer entries than the merged result needs")
        need -= min(int(p["matched"]), need)
    index = np.concatenate([np.asarray(p["index"], dtype=np.uint64) for p in parts])[:capacity]
    syn = np.concatenate([np.ascontiguousarray(p["syn"], dtype=SYN_DTYPE) for p in parts])[:capacity]
    out.update(written=int(len(index)), syn_offset=int(parts[0]["syn_offset"]), capacity=capacity,
               index=index, syn=syn)
    return out
