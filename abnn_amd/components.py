"""Connected components (abnn.h ``abnn_components_*``) on the host side.

The labelling itself runs in the HIP library (csrc/components.hip); this module
holds what needs no GPU: the config, the decoding of a result into a dict, a
numpy restatement over interchange records (:func:`reference`: the test
reference, and usable for small brains) and the shard merge on host planes
(:func:`merge`).  The reference is written independently of the C rule: not a
union-find but the fixed point of "every neuron takes the smallest label among
its neighbours", sped up by pointer jumping.  Labels are the smallest neuron id
of each component and every word is an integer, so :func:`reference` equals
the device word for word.
"""
from __future__ import annotations

from typing import Iterable, Optional, Sequence

import numpy as np

from ._lib import (COMP_BEGIN, COMP_CLOSE, COMP_FLATTEN, COMP_HEADER_WORDS, COMP_LINK, COMP_NONE, COMP_SIZE_BINS, COMP_SIZES,
                   COMP_WEIGHT, ComponentsConfig)

F32 = np.float32
U32 = np.uint32
NONE = COMP_NONE
BEGIN, LINK, FLATTEN, CLOSE = COMP_BEGIN, COMP_LINK, COMP_FLATTEN, COMP_CLOSE
PLANE_AT = COMP_HEADER_WORDS + COMP_SIZE_BINS  # the u64 word at which the label plane starts
_COUNT_KEYS = ("records", "neurons", "followed", "components", "largest", "largest_label", "singletons", "gave_up")  # words 0..7
_ALL = COMP_WEIGHT | COMP_SIZES


def config(neurons: Optional[Sequence[int]] = None, weights: Optional[Sequence[float]] = None, sizes: bool = False,
           n_nrn: Optional[int] = None) -> ComponentsConfig:
    """``neurons`` is the (first, count) range R whose components are asked
    (None: every neuron, which needs ``n_nrn``); ``weights`` = (w_lo, w_hi)
    follows only records with w_lo <= w < w_hi (inf allowed); ``sizes`` also
    returns the per-neuron component-size plane."""
    if neurons is None:
        if n_nrn is None:
            raise ValueError("components.config: neurons=None needs n_nrn")
        neurons = (0, int(n_nrn))
    lo, hi = (0.0, 0.0) if weights is None else (float(weights[0]), float(weights[1]))
    flags = (COMP_WEIGHT if weights is not None else 0) | (COMP_SIZES if sizes else 0)
    return ComponentsConfig(int(neurons[0]), int(neurons[1]), flags, lo, hi)  # reserved: zeros


def _bits(x: float) -> int:
    return int(np.array([x], dtype=F32).view(U32)[0])


def config_ok(cfg: Optional[ComponentsConfig], n_nrn: int) -> bool:
    """The checks of abnn_components_words."""
    n_nrn = int(n_nrn)
    if cfg is None or n_nrn <= 0 or n_nrn >= 1 << 32 or cfg.flags & ~_ALL or any(cfg.reserved):
        return False
    if cfg.count == 0 or cfg.first + cfg.count > n_nrn:
        return False
    if cfg.flags & COMP_WEIGHT:
        if not F32(cfg.w_lo) < F32(cfg.w_hi):  # false for a NaN bound
            return False
    elif _bits(cfg.w_lo) or _bits(cfg.w_hi):
        return False
    return True


def n_words(cfg: ComponentsConfig, n_nrn: int) -> int:
    """abnn_components_words: 8 + 32 + (N_NRN + 1) // 2, with SIZES as many
    again for the size plane, or 0 for an invalid config."""
    if not config_ok(cfg, n_nrn):
        return 0
    return PLANE_AT + (int(n_nrn) + 1) // 2 * (2 if cfg.flags & COMP_SIZES else 1)


def followed(syn: np.ndarray, cfg: ComponentsConfig, n_nrn: int) -> np.ndarray:
    """The rule of abnn.h over interchange records: a bool per record."""
    src, dst = syn["src"].astype(np.int64), syn["dst"].astype(np.int64)
    lo, hi = int(cfg.first), int(cfg.first) + int(cfg.count)
    m = (dst != 0xFFFFFFFF) & (src >= lo) & (src < hi) & (dst >= lo) & (dst < hi)
    if cfg.flags & COMP_WEIGHT:
        w = syn["w"].astype(F32)
        with np.errstate(invalid="ignore"):
            m &= (w >= F32(cfg.w_lo)) & (w < F32(cfg.w_hi))  # false for NaN
    return m


def _jump(lab: np.ndarray) -> np.ndarray:
    while True:
        nxt = lab[lab]
        if np.array_equal(nxt, lab):
            return lab
        lab = nxt


def _min_labels(u: np.ndarray, v: np.ndarray, n: int) -> np.ndarray:
    """The fixed point of lab[x] = min(lab[x], lab[y] over x's neighbours y),
    from lab[x] = x: the smallest id of x's component.  Each round lowers the
    label of both ends' current labels and of both ends to the smaller one,
    then jumps the pointers until lab[lab] == lab."""
    lab = np.arange(n, dtype=np.int64)
    while True:
        lu, lv = lab[u], lab[v]
        m = np.minimum(lu, lv)
        new = lab.copy()
        for at in (lu, lv, u, v):
            np.minimum.at(new, at, m)
        new = _jump(new)
        if np.array_equal(new, lab):
            return lab
        lab = new


def close(labels: np.ndarray, cfg: ComponentsConfig, records: int, n_followed: int) -> dict:
    """The result dict from a finished label plane (NONE outside R)."""
    labels = np.ascontiguousarray(labels, dtype=U32)
    n_nrn = len(labels)
    lo, hi = int(cfg.first), int(cfg.first) + int(cfg.count)
    ids, counts = np.unique(labels[lo:hi], return_counts=True)  # ids ascend
    at = int(np.argmax(counts))  # the first of the largest: the smallest label
    bins = np.bincount(np.frexp(counts.astype(np.float64))[1].astype(np.int64) - 1, minlength=COMP_SIZE_BINS).astype(np.uint64)
    d = {"records": int(records), "neurons": n_nrn, "followed": int(n_followed), "components": int(len(ids)),
         "largest": int(counts[at]), "largest_label": int(ids[at]), "singletons": int((counts == 1).sum()), "gave_up": 0,
         "bins": bins, "labels": labels}
    if cfg.flags & COMP_SIZES:
        size_of = np.zeros(n_nrn, dtype=U32)
        size_of[ids.astype(np.int64)] = counts.astype(U32)
        sizes = np.zeros(n_nrn, dtype=U32)
        sizes[lo:hi] = size_of[labels[lo:hi].astype(np.int64)]
        d["sizes"] = sizes
    return d


def reference(syn: np.ndarray, cfg: ComponentsConfig, n_nrn: int) -> dict:
    """The labelling over interchange records ``syn`` (fields src, dst, w) in
    numpy: the header counts, ``bins`` (np.uint64, 32), ``labels`` (np.uint32,
    N_NRN; NONE outside R) and, with SIZES, ``sizes`` (np.uint32)."""
    if not config_ok(cfg, n_nrn):
        raise ValueError("components: invalid config")
    m = followed(syn, cfg, n_nrn)
    u, v = syn["src"][m].astype(np.int64), syn["dst"][m].astype(np.int64)
    lab = _min_labels(u, v, int(n_nrn))
    labels = np.full(int(n_nrn), NONE, dtype=U32)
    lo, hi = int(cfg.first), int(cfg.first) + int(cfg.count)
    labels[lo:hi] = lab[lo:hi]  # no followed record leaves R: a label of R is in R
    return close(labels, cfg, len(syn), int(m.sum()))


def merge(planes: Iterable[np.ndarray], cfg: ComponentsConfig) -> np.ndarray:
    """The shard merge on host planes: the label plane of the union of the
    graphs whose label planes are given (each a spanning forest of its graph:
    n -- planes[p][n]).  An entry that is NONE or not in R is skipped."""
    planes = [np.asarray(p, dtype=U32) for p in planes]
    if not planes:
        raise ValueError("merge: no planes")
    n_nrn = len(planes[0])
    lo, hi = int(cfg.first), int(cfg.first) + int(cfg.count)
    us, vs = [], []
    for p in planes:
        if p.shape != (n_nrn,):
            raise ValueError("merge: planes of different sizes")
        n = np.arange(lo, hi, dtype=np.int64)
        l = p[lo:hi].astype(np.int64)
        ok = (l >= lo) & (l < hi)
        us.append(n[ok])
        vs.append(l[ok])
    lab = _min_labels(np.concatenate(us), np.concatenate(vs), n_nrn)
    out = np.full(n_nrn, NONE, dtype=U32)
    out[lo:hi] = lab[lo:hi]
    return out


def decode(words: np.ndarray, cfg: ComponentsConfig, n_nrn: int) -> dict:
    """A result's u64 words (abnn.h) as a dict: the header counts, ``bins``
    (np.uint64), ``labels`` (np.uint32) and, with SIZES, ``sizes``."""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    assert n_words(cfg, n_nrn) and w.shape == (n_words(cfg, n_nrn),), (w.shape, n_nrn)
    d = {k: int(w[i]) for i, k in enumerate(_COUNT_KEYS)}
    pw = (int(n_nrn) + 1) // 2
    d["bins"] = w[COMP_HEADER_WORDS:PLANE_AT].copy()
    d["labels"] = w[PLANE_AT:PLANE_AT + pw].view(U32)[:int(n_nrn)].copy()
    if cfg.flags & COMP_SIZES:
        d["sizes"] = w[PLANE_AT + pw:].view(U32)[:int(n_nrn)].copy()
    return d


def _plane_words(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=U32)
    plane = np.zeros((len(a) + 1) // 2 * 2, dtype=U32)
    plane[:len(a)] = a
    return plane.view(np.uint64)


def to_words(d: dict) -> np.ndarray:
    """The inverse of :func:`decode`: the result's u64 words (the pad entry of
    an odd N_NRN is 0)."""
    head = np.array([d[k] for k in _COUNT_KEYS], dtype=np.uint64)
    parts = [head, np.ascontiguousarray(d["bins"], dtype=np.uint64), _plane_words(d["labels"])]
    if "sizes" in d:
        parts.append(_plane_words(d["sizes"]))
    return np.concatenate(parts)
