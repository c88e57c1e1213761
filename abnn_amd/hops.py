"""Reachability (abnn.h ``abnn_hops_*``) on the host side.

The search itself runs in the HIP library (csrc/hops.hip); this module holds
what needs no GPU: the config, the decoding of a result into a dict, the numpy
restatement of the steps over interchange records (:func:`begin`, :func:`step`
and :func:`reference`: the test reference, and usable for small brains) and
the merge of the shards' planes between two steps (:func:`merge_planes`).
Distances are breadth-first levels and every word is an integer, so
:func:`reference` equals the device word for word.
"""
from __future__ import annotations

from typing import Iterable, Optional, Sequence

import numpy as np

from ._lib import (HOPS_BEGIN, HOPS_HEADER_WORDS, HOPS_MAX, HOPS_REVERSE, HOPS_UNREACHED, HOPS_WEIGHT, HopsConfig)

F32 = np.float32
U32 = np.uint32
UNREACHED = HOPS_UNREACHED
BEGIN = HOPS_BEGIN
# csrc/hops.h kHopsFoldWords / kHopsFoldMaxFrontier: the expand kernel tests records against an LDS fold of
# the frontier bitmap (FOLD_WORDS u32) when the frontier holds at most FOLD_MAX_FRONTIER neurons or the whole
# bitmap fits the fold, and against the bitmap itself otherwise
FOLD_WORDS = 8192
FOLD_MAX_FRONTIER = 32 * FOLD_WORDS // 8
_COUNT_KEYS = ("records", "neurons", "reached", "depth", "complete")  # words 0..4
_ALL = HOPS_REVERSE | HOPS_WEIGHT


def config(seeds: Sequence[int], max_hops: int = 64, reverse: bool = False,
           weights: Optional[Sequence[float]] = None) -> HopsConfig:
    """``seeds`` is the (first, count) neuron range the search starts from;
    ``reverse`` follows dst -> src (who can reach the seeds); ``weights`` =
    (w_lo, w_hi) follows only records with w_lo <= w < w_hi (inf allowed)."""
    lo, hi = (0.0, 0.0) if weights is None else (float(weights[0]), float(weights[1]))
    flags = (HOPS_REVERSE if reverse else 0) | (HOPS_WEIGHT if weights is not None else 0)
    return HopsConfig(int(seeds[0]), int(seeds[1]), int(max_hops), flags, lo, hi)  # reserved: zeros


def _bits(x: float) -> int:
    return int(np.array([x], dtype=F32).view(U32)[0])


def config_ok(cfg: Optional[HopsConfig], n_nrn: int) -> bool:
    """The checks of abnn_hops_words."""
    n_nrn = int(n_nrn)
    if cfg is None or n_nrn <= 0 or cfg.flags & ~_ALL or any(cfg.reserved):
        return False
    if cfg.seed_count == 0 or cfg.seed_first + cfg.seed_count > n_nrn:
        return False
    if not 1 <= cfg.max_hops <= HOPS_MAX:
        return False
    if cfg.flags & HOPS_WEIGHT:
        if not F32(cfg.w_lo) < F32(cfg.w_hi):  # false for a NaN bound
            return False
    elif _bits(cfg.w_lo) or _bits(cfg.w_hi):
        return False
    return True


def n_words(cfg: HopsConfig, n_nrn: int) -> int:
    """abnn_hops_words: 8 + (H + 1) + (N_NRN + 1) // 2, or 0 for an invalid config."""
    if not config_ok(cfg, n_nrn):
        return 0
    return HOPS_HEADER_WORDS + int(cfg.max_hops) + 1 + (int(n_nrn) + 1) // 2


def plane_offset(cfg: HopsConfig) -> int:
    """The u64 word at which the distance plane starts."""
    return HOPS_HEADER_WORDS + int(cfg.max_hops) + 1


def followed(syn: np.ndarray, cfg: HopsConfig, n_nrn: int) -> np.ndarray:
    """The rule of abnn.h over interchange records: a bool per record."""
    src, dst = syn["src"].astype(U32), syn["dst"].astype(U32)
    m = (dst != U32(0xFFFFFFFF)) & (src < U32(n_nrn)) & (dst < U32(n_nrn))
    if cfg.flags & HOPS_WEIGHT:
        w = syn["w"].astype(F32)
        with np.errstate(invalid="ignore"):
            m &= (w >= F32(cfg.w_lo)) & (w < F32(cfg.w_hi))  # false for NaN
    return m


def edges(syn: np.ndarray, cfg: HopsConfig, n_nrn: int) -> tuple[np.ndarray, np.ndarray]:
    """(u, v) of the followed records, in the direction of the search."""
    m = followed(syn, cfg, n_nrn)
    src, dst = syn["src"][m].astype(np.int64), syn["dst"][m].astype(np.int64)
    return (dst, src) if cfg.flags & HOPS_REVERSE else (src, dst)


def begin(cfg: HopsConfig, n_nrn: int) -> tuple[np.ndarray, np.ndarray]:
    """Step BEGIN: (levels, plane) -- the levels zero, the plane 0 on the seeds
    and UNREACHED elsewhere."""
    if not config_ok(cfg, n_nrn):
        raise ValueError("hops: invalid config")
    plane = np.full(int(n_nrn), UNREACHED, dtype=U32)
    plane[cfg.seed_first:cfg.seed_first + cfg.seed_count] = 0
    return np.zeros(int(cfg.max_hops) + 1, dtype=np.uint64), plane


def step(uv: tuple[np.ndarray, np.ndarray], cfg: HopsConfig, levels: np.ndarray, plane: np.ndarray, h: int) -> None:
    """Step ``h`` (0 .. H) over the edges ``uv`` (:func:`edges`), in place:
    nothing when h > 0 and levels[h-1] == 0; else levels[h] is counted from
    the plane and, for h < H, every edge out of distance h sets its target to
    at most h + 1."""
    h = int(h)
    if not 0 <= h <= cfg.max_hops:
        raise ValueError("hops: a step is 0 .. max_hops")
    if h > 0 and levels[h - 1] == 0:
        return
    levels[h] = int((plane == U32(h)).sum())
    if h == cfg.max_hops:
        return
    u, v = uv
    targets = v[plane[u] == U32(h)]
    plane[targets] = np.minimum(plane[targets], U32(h + 1))  # one value: duplicates are harmless


def close(cfg: HopsConfig, levels: np.ndarray, plane: np.ndarray, records: int) -> dict:
    """The result dict of finished steps (the header words 0..4 from the levels)."""
    nz = np.flatnonzero(levels)
    return {"records": int(records), "neurons": int(len(plane)), "reached": int(levels.sum()),
            "depth": int(nz[-1]) if len(nz) else 0, "complete": int(levels[cfg.max_hops] == 0),
            "levels": levels.astype(np.uint64), "dist": plane.astype(U32)}


def reference(syn: np.ndarray, cfg: HopsConfig, n_nrn: int) -> dict:
    """The search over interchange records ``syn`` (fields src, dst, w) in
    numpy: records, neurons, reached, depth, complete, ``levels`` (np.uint64,
    H + 1) and ``dist`` (np.uint32, N_NRN; UNREACHED = not within H hops)."""
    levels, plane = begin(cfg, n_nrn)
    uv = edges(syn, cfg, n_nrn)
    for h in range(int(cfg.max_hops) + 1):
        if h > 0 and levels[h - 1] == 0:
            break  # every later step is dead
        step(uv, cfg, levels, plane, h)
    return close(cfg, levels, plane, len(syn))


def merge_planes(parts: Iterable[np.ndarray]) -> np.ndarray:
    """The element-wise minimum of the ranks' planes: what a sharded caller
    puts into every rank's plane between two steps."""
    parts = [np.asarray(p, dtype=U32) for p in parts]
    if not parts:
        raise ValueError("merge_planes: no planes")
    out = parts[0].copy()
    for p in parts[1:]:
        if p.shape != out.shape:
            raise ValueError("merge_planes: planes of different sizes")
        np.minimum(out, p, out=out)
    return out


def decode(words: np.ndarray, cfg: HopsConfig, n_nrn: int) -> dict:
    """A result's u64 words (abnn.h) as a dict: the header counts, ``levels``
    (np.uint64) and ``dist`` (np.uint32)."""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    assert n_words(cfg, n_nrn) and w.shape == (n_words(cfg, n_nrn),), (w.shape, n_nrn)
    d = {k: int(w[i]) for i, k in enumerate(_COUNT_KEYS)}
    at = plane_offset(cfg)
    d["levels"] = w[HOPS_HEADER_WORDS:at].copy()
    d["dist"] = w[at:].view(U32)[:int(n_nrn)].copy()
    return d


def to_words(d: dict) -> np.ndarray:
    """The inverse of :func:`decode`: the result's u64 words (the pad entry of
    an odd N_NRN is 0)."""
    dist = np.ascontiguousarray(d["dist"], dtype=U32)
    plane = np.zeros((len(dist) + 1) // 2 * 2, dtype=U32)
    plane[:len(dist)] = dist
    head = np.array([d[k] for k in _COUNT_KEYS] + [0, 0, 0], dtype=np.uint64)
    return np.concatenate([head, np.ascontiguousarray(d["levels"], dtype=np.uint64), plane.view(np.uint64)])
