"""The synapse census (abnn.h ``abnn_census_*``) on the host side.

The census itself runs in the HIP library (csrc/census.hip); this module holds
what needs no GPU: the config, the decoding of a result into a dict, the numpy
restatement of the definition over interchange records (:func:`reference`: the
test reference, and usable for small brains) and the merge of several results
(:func:`merge`: shards).  Every count is an integer and every float operation
a single float32 operation, so :func:`reference` equals the device bit for bit.
"""
from __future__ import annotations

from typing import Iterable, Optional, Sequence

import numpy as np

from ._lib import CENSUS_HEADER_WORDS, CENSUS_MAX_BINS, CensusConfig

F32 = np.float32
_COUNT_KEYS = ("records", "tombstones", "selected", "under", "over", "nan")  # words 0..5 (live is derived)


def config(bins: int, lo: float, hi: float, src: Optional[Sequence[int]] = None,
           dst: Optional[Sequence[int]] = None) -> CensusConfig:
    """``src`` / ``dst`` are (first, count) pairs; None (or count 0) = any."""
    s = (0, 0) if src is None else (int(src[0]), int(src[1]))
    d = (0, 0) if dst is None else (int(dst[0]), int(dst[1]))
    return CensusConfig(float(lo), float(hi), int(bins), s[0], s[1], d[0], d[1], 0)


def _scale(cfg: CensusConfig) -> np.float32:
    """(float)bins / (hi - lo) in float32, or ValueError for what abnn_census_words refuses."""
    lo, hi = F32(cfg.lo), F32(cfg.hi)
    if not 1 <= cfg.bins <= CENSUS_MAX_BINS or cfg.reserved != 0:
        raise ValueError("census: bins must be 1..4096 and reserved 0")
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError("census: lo < hi, both finite")
    with np.errstate(over="ignore", divide="ignore"):
        span = hi - lo
        scale = F32(cfg.bins) / span
    if not (np.isfinite(span) and np.isfinite(scale)):
        raise ValueError("census: hi - lo and bins / (hi - lo) must be finite in float32")
    return scale


def n_words(cfg: CensusConfig) -> int:
    """abnn_census_words: 8 + bins, or 0 for an invalid config."""
    try:
        _scale(cfg)
    except ValueError:
        return 0
    return CENSUS_HEADER_WORDS + int(cfg.bins)


def edges(cfg: CensusConfig) -> np.ndarray:
    """bins + 1 nominal bin edges (float64).  The bin of a weight is defined
    by the float32 formula of abnn.h, which may differ from these by a rounding."""
    return float(cfg.lo) + (float(cfg.hi) - float(cfg.lo)) * np.arange(cfg.bins + 1, dtype=np.float64) / cfg.bins


def _bits_f32(word: int) -> np.float32:
    return np.array([int(word) & 0xFFFFFFFF], dtype=np.uint32).view(F32)[0]


def _f32_bits(x) -> int:
    return int(np.array([x], dtype=F32).view(np.uint32)[0])


def order_key(bits) -> np.ndarray:
    """The total order of float32 bit patterns used for min / max (-0.0 < +0.0)."""
    b = np.asarray(bits, dtype=np.uint32)
    return np.where(b >> np.uint32(31), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def decode(words: np.ndarray, cfg: CensusConfig) -> dict:
    """A result's u64 words (abnn.h) as a dict."""
    w = np.asarray(words, dtype=np.uint64)
    assert w.shape == (CENSUS_HEADER_WORDS + cfg.bins,), w.shape
    d = {k: int(w[i]) for i, k in enumerate(_COUNT_KEYS)}
    d["live"] = d["records"] - d["tombstones"]
    d["min"], d["max"] = _bits_f32(w[6]), _bits_f32(w[7])
    d["counts"] = w[CENSUS_HEADER_WORDS:].copy()
    d["edges"] = edges(cfg)
    return d


def to_words(d: dict) -> np.ndarray:
    """The inverse of :func:`decode`: the result's u64 words."""
    head = [d[k] for k in _COUNT_KEYS] + [_f32_bits(d["min"]), _f32_bits(d["max"])]
    return np.concatenate([np.array(head, dtype=np.uint64), np.asarray(d["counts"], dtype=np.uint64)])


def reference(syn: np.ndarray, cfg: CensusConfig) -> dict:
    """The census of interchange records ``syn`` (fields src, dst, w) in numpy."""
    scale = _scale(cfg)
    lo, hi, bins = F32(cfg.lo), F32(cfg.hi), int(cfg.bins)
    src, dst = syn["src"].astype(np.uint32), syn["dst"].astype(np.uint32)
    tomb = dst == np.uint32(0xFFFFFFFF)
    sel = ~tomb
    for x, first, count in ((src, cfg.src_first, cfg.src_count), (dst, cfg.dst_first, cfg.dst_count)):
        if count:
            sel &= (x.astype(np.int64) >= first) & (x.astype(np.int64) < first + count)
    ws = np.ascontiguousarray(syn["w"][sel], dtype=F32)
    is_nan = ws != ws
    v = ws[~is_nan]
    under, over = v < lo, v >= hi
    mid = v[~under & ~over]
    idx = np.minimum(((mid - lo) * scale).astype(np.uint32), np.uint32(bins - 1))
    d = {"records": int(len(syn)), "tombstones": int(tomb.sum()), "selected": int(sel.sum()),
         "under": int(under.sum()), "over": int(over.sum()), "nan": int(is_nan.sum())}
    d["live"] = d["records"] - d["tombstones"]
    if len(v):
        key = order_key(v.view(np.uint32))
        d["min"], d["max"] = v[int(np.argmin(key))], v[int(np.argmax(key))]
    else:
        d["min"], d["max"] = F32(np.inf), F32(-np.inf)
    d["counts"] = np.bincount(idx, minlength=bins).astype(np.uint64)
    d["edges"] = edges(cfg)
    return d


def merge(results: Iterable[dict]) -> dict:
    """The census of the union of disjoint record sets (shards) from their
    censuses under one config: counts and bins add, min and max combine in
    the order of :func:`order_key`."""
    results = list(results)
    if not results:
        raise ValueError("merge: no results")
    out = {k: sum(int(r[k]) for r in results) for k in _COUNT_KEYS}
    out["live"] = out["records"] - out["tombstones"]
    out["min"] = min((r["min"] for r in results), key=lambda x: int(order_key(_f32_bits(x))))
    out["max"] = max((r["max"] for r in results), key=lambda x: int(order_key(_f32_bits(x))))
    counts = np.zeros_like(np.asarray(results[0]["counts"], dtype=np.uint64))
    for r in results:
        if len(r["counts"]) != len(counts):
            raise ValueError("merge: results of different configs")
        counts += np.asarray(r["counts"], dtype=np.uint64)
    out["counts"] = counts
    out["edges"] = np.array(results[0]["edges"], copy=True)
    return out
