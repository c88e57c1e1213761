"""Population connectivity matrix (abnn.h ``abnn_matrix_*``) on the host side.

The scan itself runs in the HIP library (csrc/matrix.hip); this module holds
what needs no GPU: the config, the built-in populations' bounds, the decoding
of a result into a dict, a numpy restatement over interchange records
(:func:`reference`: the test reference, and usable for small brains) and the
merge of shard results (:func:`merge`).  Every word is an integer sum, so
:func:`reference` equals the device word for word.
"""
from __future__ import annotations

from typing import Iterable, Optional, Sequence

import numpy as np

from ._lib import (MAT_COUNT, MAT_LABELS, MAT_P, MAT_W, MAT_WEIGHT, MATRIX_HEADER_WORDS, MATRIX_MAX_POPS, MatrixConfig)

F32 = np.float32
U32 = np.uint32
U64 = np.uint64
I64 = np.int64
ONE = 1 << 24  # the fixed point of the W and P planes
COUNT, W, P = MAT_COUNT, MAT_W, MAT_P
SIZES_AT = MATRIX_HEADER_WORDS
_WHAT = {"count": MAT_COUNT, "w": MAT_W, "p": MAT_P}
_HEAD_KEYS = ("records", "tombstones", "counted", "src_unassigned", "dst_unassigned", "unassigned", "out_of_band",
              "skipped_w", "skipped_p", "pops", "neurons", "assigned")  # words 0..11
_SUMMED = 9  # words 0..8 add up over shards


def config(pops: int, what=("count",), labels: bool = False, weights: Optional[Sequence[float]] = None) -> MatrixConfig:
    """``pops`` populations; ``what`` names the planes ("count", "w", "p", or
    the bit mask); ``labels`` = the partition is a label plane, not bounds;
    ``weights`` = (w_lo, w_hi) counts only records with w_lo <= w < w_hi."""
    bits = int(what) if isinstance(what, (int, np.integer)) else sum({_WHAT[k] for k in what})
    lo, hi = (0.0, 0.0) if weights is None else (float(weights[0]), float(weights[1]))
    flags = (MAT_LABELS if labels else 0) | (MAT_WEIGHT if weights is not None else 0)
    return MatrixConfig(int(pops), bits, flags, lo, hi)  # reserved: zeros


def _bits(x: float) -> int:
    return int(np.array([x], dtype=F32).view(U32)[0])


def config_ok(cfg: Optional[MatrixConfig]) -> bool:
    """The checks of abnn_matrix_words."""
    if cfg is None or not 1 <= cfg.pops <= MATRIX_MAX_POPS or any(cfg.reserved):
        return False
    if cfg.what == 0 or cfg.what & ~(COUNT | W | P) or cfg.flags & ~(MAT_LABELS | MAT_WEIGHT):
        return False
    if cfg.flags & MAT_WEIGHT:
        if not F32(cfg.w_lo) < F32(cfg.w_hi):  # false for a NaN bound
            return False
    elif _bits(cfg.w_lo) or _bits(cfg.w_hi):
        return False
    return True


def n_planes(cfg: MatrixConfig) -> int:
    return bin(cfg.what & (COUNT | W | P)).count("1")


def n_words(cfg: MatrixConfig) -> int:
    """abnn_matrix_words: 16 + P + planes * P * P, or 0 for an invalid config."""
    if not config_ok(cfg):
        return 0
    return SIZES_AT + cfg.pops + n_planes(cfg) * cfg.pops * cfg.pops


def bounds_ok(bounds, pops: int, n_nrn: int) -> bool:
    """bounds[0] <= ... <= bounds[P] <= n_nrn, P + 1 values."""
    b = np.asarray(bounds, dtype=I64)
    return b.shape == (int(pops) + 1,) and bool((np.diff(b) >= 0).all()) and 0 <= int(b[0]) and int(b[-1]) <= int(n_nrn)


def io_bounds(n_in: int, n_out: int, n_hidden: int) -> np.ndarray:
    """The bounds of a handle's built-in populations in its id order: inputs
    [0, n_in), outputs [n_in, n_in + n_out), hidden the rest (P = 3)."""
    return np.array([0, n_in, n_in + n_out, n_in + n_out + n_hidden], dtype=U32)


def pops_of(ids: np.ndarray, cfg: MatrixConfig, n_nrn: int, bounds=None, labels=None) -> np.ndarray:
    """pop(n) of abnn.h for an array of ids: 0 .. P - 1, or -1 for none."""
    ids = np.asarray(ids).astype(I64)
    if cfg.flags & MAT_LABELS:
        lab = np.asarray(labels, dtype=U32).astype(I64)
        ok = ids < int(n_nrn)
        v = lab[np.where(ok, ids, 0)]
        return np.where(ok & (v < cfg.pops), v, -1)
    b = np.asarray(bounds, dtype=U32).astype(I64)
    j = np.searchsorted(b, ids, side="right") - 1  # the last j with bounds[j] <= n
    return np.where((ids >= b[0]) & (ids < b[-1]), j, -1)


def terms(c: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """The fixed-point terms of fp32 coefficients: (q as int64, summable)."""
    c = np.asarray(c, dtype=F32)
    with np.errstate(invalid="ignore"):
        summable = np.abs(c) < F32(128.0)  # false for NaN and +-inf
    q = (np.where(summable, c, F32(0)) * F32(16777216.0)).astype(np.int32)  # exact product, truncation toward zero
    return q.astype(I64), summable


def _plane(cells: np.ndarray, v: np.ndarray, pops: int) -> np.ndarray:
    out = np.zeros(pops * pops, dtype=U64)
    np.add.at(out, cells, v.astype(I64).view(U64))  # modulo 2**64
    return out.reshape(pops, pops)


def reference(records: np.ndarray, cfg: MatrixConfig, n_nrn: int, base_scale: float = 0.0, bounds=None, labels=None) -> dict:
    """The rule of abnn.h over interchange records (fields src, dst, w) in
    numpy: the header as ints, ``sizes`` (np.uint64, P) and the planes asked
    (``count`` np.uint64, ``w`` / ``p`` np.int64, each (P, P))."""
    if not config_ok(cfg) or not 1 <= int(n_nrn) < 1 << 32:
        raise ValueError("matrix: invalid config")
    lab = bool(cfg.flags & MAT_LABELS)
    if lab != (labels is not None) or lab == (bounds is not None):
        raise ValueError("matrix: exactly one of bounds / labels, the one the LABELS flag names")
    pops = int(cfg.pops)
    if lab:
        labels = np.ascontiguousarray(labels, dtype=U32)
        if labels.shape != (int(n_nrn),):
            raise ValueError("matrix: labels must hold N_NRN entries")
        sizes = np.bincount(labels[labels < pops].astype(I64), minlength=pops).astype(U64)
    else:
        if not bounds_ok(bounds, pops, n_nrn):
            raise ValueError("matrix: bounds must ascend and end at or below N_NRN")
        sizes = np.diff(np.asarray(bounds, dtype=I64)).astype(U64)
    src, dst, w = records["src"].astype(U32), records["dst"].astype(U32), records["w"].astype(F32)
    live = dst != U32(0xFFFFFFFF)
    band = np.ones(len(records), dtype=bool)
    if cfg.flags & MAT_WEIGHT:
        with np.errstate(invalid="ignore"):
            band = (w >= F32(cfg.w_lo)) & (w < F32(cfg.w_hi))  # false for NaN
    use = live & band
    a = pops_of(src, cfg, n_nrn, bounds, labels)
    b = pops_of(dst, cfg, n_nrn, bounds, labels)
    counted = use & (a >= 0) & (b >= 0)
    cells = (a[counted] * pops + b[counted]).astype(I64)
    d = {"records": int(len(records)), "tombstones": int((~live).sum()), "counted": int(counted.sum()),
         "src_unassigned": int((use & (a < 0) & (b >= 0)).sum()), "dst_unassigned": int((use & (a >= 0) & (b < 0)).sum()),
         "unassigned": int((use & (a < 0) & (b < 0)).sum()), "out_of_band": int((live & ~band).sum()),
         "skipped_w": 0, "skipped_p": 0, "pops": pops, "neurons": int(n_nrn), "assigned": int(sizes.sum()), "sizes": sizes}
    wc = w[counted]
    if cfg.what & COUNT:
        d["count"] = _plane(cells, np.ones(len(cells), dtype=I64), pops)
    if cfg.what & W:
        q, ok = terms(wc)
        d["skipped_w"] = int((~ok).sum())
        d["w"] = _plane(cells[ok], q[ok], pops).view(I64)
    if cfg.what & P:
        with np.errstate(over="ignore", invalid="ignore"):
            c = (wc * wc) * F32(base_scale)  # two fp32 operations
        q, ok = terms(c)
        d["skipped_p"] = int((~ok).sum())
        d["p"] = _plane(cells[ok], q[ok], pops).view(I64)
    return d


def to_words(d: dict) -> np.ndarray:
    """A result dict's u64 words (abnn.h): the inverse of :func:`decode`."""
    head = np.zeros(SIZES_AT, dtype=U64)
    head[:len(_HEAD_KEYS)] = [d[k] for k in _HEAD_KEYS]
    parts = [head, np.ascontiguousarray(d["sizes"], dtype=U64)]
    for k in ("count", "w", "p"):
        if k in d:
            parts.append(np.ascontiguousarray(d[k]).view(U64).reshape(-1))
    return np.concatenate(parts)


def decode(words: np.ndarray, cfg: MatrixConfig) -> dict:
    """A result's u64 words as a dict: the header as ints, ``sizes``, the
    planes asked as (P, P) arrays (``count`` np.uint64, ``w`` / ``p`` np.int64
    in 2**-24 fixed point, with ``w_float`` / ``p_float`` = the same / 2**24)
    and ``density`` = count / (sizes[a] * sizes[b]) (nan for an empty pair)
    when COUNT was asked."""
    wd = np.ascontiguousarray(words, dtype=U64)
    assert n_words(cfg) and wd.shape == (n_words(cfg),), (wd.shape, n_words(cfg))
    pops = int(cfg.pops)
    d = {k: int(wd[i]) for i, k in enumerate(_HEAD_KEYS)}
    d["sizes"] = wd[SIZES_AT:SIZES_AT + pops].copy()
    at = SIZES_AT + pops
    for k, bit in (("count", COUNT), ("w", W), ("p", P)):
        if cfg.what & bit:
            plane = wd[at:at + pops * pops].reshape(pops, pops).copy()
            d[k] = plane if k == "count" else plane.view(I64)
            at += pops * pops
    for k in ("w", "p"):
        if k in d:
            d[k + "_float"] = d[k].astype(np.float64) / ONE
    if "count" in d:
        pairs = np.outer(d["sizes"].astype(np.float64), d["sizes"].astype(np.float64))
        with np.errstate(divide="ignore", invalid="ignore"):
            d["density"] = d["count"].astype(np.float64) / pairs
    return d


def merge_words(parts: Iterable[np.ndarray]) -> np.ndarray:
    """The shard merge on result words: words 0..8 and the planes are summed
    (modulo 2**64); words 9..15 and the sizes are the first part's (they are
    the same on every rank)."""
    parts = [np.ascontiguousarray(p, dtype=U64) for p in parts]
    if not parts:
        raise ValueError("merge: no parts")
    out = parts[0].copy()
    pops = int(out[9])
    for p in parts[1:]:
        if p.shape != out.shape or not np.array_equal(p[_SUMMED:SIZES_AT + pops], out[_SUMMED:SIZES_AT + pops]):
            raise ValueError("merge: parts of different partitions")
        out[:_SUMMED] += p[:_SUMMED]
        out[SIZES_AT + pops:] += p[SIZES_AT + pops:]
    return out


def merge(parts: Iterable[dict]) -> dict:
    """The shard merge on result dicts (of :func:`reference` or :func:`decode`):
    the planes asked are those of the first part."""
    parts = list(parts)
    if not parts:
        raise ValueError("merge: no parts")
    what = sum(bit for k, bit in _WHAT.items() if k in parts[0])
    cfg = MatrixConfig(int(parts[0]["pops"]), what, 0, 0.0, 0.0)
    return decode(merge_words([to_words(p) for p in parts]), cfg)
