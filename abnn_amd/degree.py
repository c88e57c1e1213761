"""The neuron degree census (abnn.h ``abnn_degree_*``) on the host side.

The census itself runs in the HIP library (csrc/degree.hip); this module holds
what needs no GPU: the config, the decoding of a result into a dict, the numpy
restatement of the definition over interchange records (:func:`reference`: the
test reference, and usable for small brains) and the merge of several results
(:func:`merge`: shards).  Every word is an integer sum and a weight's term one
float32 multiply (exact) and a truncation, so :func:`reference` equals the
device bit for bit.
"""
from __future__ import annotations

from typing import Iterable, Optional, Sequence, Union

import numpy as np

from ._lib import DEG_IN, DEG_IN_W, DEG_OUT, DEG_OUT_W, DEGREE_HEADER_WORDS, DegreeConfig

F32 = np.float32
# csrc/degree.h kDegreeNarrowMax: ranges of at most this many neurons are counted
# in LDS (the narrow path), longer ones with atomics into the result (the wide path)
NARROW_MAX = 4096
# csrc/degree.h kDegreeLdsBytes: a narrow range whose planes (8 B per strength,
# 4 B per degree and neuron) exceed it is scanned once per direction
NARROW_LDS_BYTES = 64 * 1024
FIXED_ONE = 1 << 24  # strength = int64 word / FIXED_ONE
PLANES = (("out", DEG_OUT, np.uint64), ("in", DEG_IN, np.uint64),
          ("out_w", DEG_OUT_W, np.int64), ("in_w", DEG_IN_W, np.int64))  # in increasing bit order
_COUNT_KEYS = ("records", "tombstones", "out_total", "in_total", "out_skipped", "in_skipped")  # words 0..5
_ALL = DEG_OUT | DEG_IN | DEG_OUT_W | DEG_IN_W


def what_bits(what: Union[int, Iterable[str]]) -> int:
    """Plane names ("out", "in", "out_w", "in_w") or the bits themselves."""
    if isinstance(what, (int, np.integer)):
        return int(what)
    if isinstance(what, str):
        what = (what,)
    names = {name: bit for name, bit, _ in PLANES}
    bits = 0
    for name in what:
        if name not in names:
            raise ValueError(f"degree: unknown plane {name!r}")
        bits |= names[name]
    return bits


def config(neurons: Optional[Sequence[int]] = None, what=("out", "in", "out_w", "in_w")) -> DegreeConfig:
    """``neurons`` is a (first, count) pair; None = every neuron."""
    first, count = (0, 0) if neurons is None else (int(neurons[0]), int(neurons[1]))
    return DegreeConfig(first, count, what_bits(what))  # reserved: zeros


def _count(cfg: DegreeConfig, n_nrn: int) -> int:
    """The neurons of the range, or 0 for what abnn_degree_words refuses."""
    n_nrn = int(n_nrn)
    if cfg is None or n_nrn <= 0 or cfg.what == 0 or cfg.what & ~_ALL or any(cfg.reserved):
        return 0
    if cfg.count == 0 and cfg.first != 0:
        return 0
    if cfg.first + cfg.count > n_nrn:
        return 0
    return int(cfg.count) if cfg.count else n_nrn


def n_words(cfg: DegreeConfig, n_nrn: int) -> int:
    """abnn_degree_words: 8 + planes * neurons, or 0 for an invalid config."""
    m = _count(cfg, n_nrn)
    return DEGREE_HEADER_WORDS + bin(cfg.what).count("1") * m if m else 0


def decode(words: np.ndarray, cfg: DegreeConfig, n_nrn: int) -> dict:
    """A result's u64 words (abnn.h) as a dict: the header counts, first, count
    and one array per plane asked (out / in np.uint64, out_w / in_w np.int64:
    strength = out_w / 2**24)."""
    w = np.asarray(words, dtype=np.uint64)
    m = _count(cfg, n_nrn)
    assert m and w.shape == (n_words(cfg, n_nrn),), (w.shape, m)
    d = {k: int(w[i]) for i, k in enumerate(_COUNT_KEYS)}
    d["first"], d["count"] = (int(cfg.first) if cfg.count else 0), m
    at = DEGREE_HEADER_WORDS
    for name, bit, dtype in PLANES:
        if cfg.what & bit:
            d[name] = w[at:at + m].view(dtype).copy()
            at += m
    return d


def to_words(d: dict) -> np.ndarray:
    """The inverse of :func:`decode`: the result's u64 words."""
    head = np.array([d[k] for k in _COUNT_KEYS] + [0, 0], dtype=np.uint64)
    planes = [np.ascontiguousarray(d[name]).view(np.uint64) for name, _, _ in PLANES if name in d]
    return np.concatenate([head, *planes])


def terms(w: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(summable, term) of float32 weights: summable iff |w| < 128 (false for
    NaN and inf); the term is the truncation of the float32 product w * 2**24,
    int64, 0 where not summable."""
    w = np.ascontiguousarray(w, dtype=F32)
    with np.errstate(invalid="ignore"):
        ok = np.abs(w) < F32(128.0)
    q = np.zeros(w.shape, dtype=np.int64)
    with np.errstate(under="ignore"):
        q[ok] = np.trunc(w[ok] * F32(16777216.0)).astype(np.int64)
    return ok, q


def _plane_sum(keys: np.ndarray, values: np.ndarray, m: int) -> np.ndarray:
    """Integer sums of values (int64, wrapping) per key in [0, m)."""
    out = np.zeros(m, dtype=np.int64)
    if len(keys):
        order = np.argsort(keys, kind="stable")
        k, v = keys[order], values[order]
        starts = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1]]))
        out[k[starts]] = np.add.reduceat(v, starts)
    return out


def reference(syn: np.ndarray, cfg: DegreeConfig, n_nrn: int) -> dict:
    """The degree census of interchange records ``syn`` (fields src, dst, w) in
    numpy; the strengths are summed in int64, never in floating point."""
    m = _count(cfg, n_nrn)
    if not m:
        raise ValueError("degree: invalid config")
    first = int(cfg.first) if cfg.count else 0
    src, dst = syn["src"].astype(np.int64), syn["dst"].astype(np.int64)
    live = syn["dst"].astype(np.uint32) != np.uint32(0xFFFFFFFF)
    ok, q = terms(syn["w"])
    d = {"records": int(len(syn)), "tombstones": int((~live).sum()), "out_total": 0, "in_total": 0,
         "out_skipped": 0, "in_skipped": 0, "first": first, "count": m}
    for side, x, deg_bit, w_bit in (("out", src, DEG_OUT, DEG_OUT_W), ("in", dst, DEG_IN, DEG_IN_W)):
        if not cfg.what & (deg_bit | w_bit):
            continue
        sel = live & (x >= first) & (x < first + m)
        keys = x[sel] - first
        d[side + "_total"] = int(sel.sum())
        if cfg.what & deg_bit:
            d[side] = np.bincount(keys, minlength=m).astype(np.uint64)  # integer counts: no weights
        if cfg.what & w_bit:
            d[side + "_skipped"] = int((sel & ~ok).sum())
            d[side + "_w"] = _plane_sum(keys, q[sel], m)
    return d


def merge(results: Iterable[dict]) -> dict:
    """The degree census of the union of disjoint record sets (shards) from
    their results under one config: every count and plane adds (the int64
    planes wrap, as the device's sums do)."""
    results = list(results)
    if not results:
        raise ValueError("merge: no results")
    out = {k: sum(int(r[k]) for r in results) for k in _COUNT_KEYS}
    out["first"], out["count"] = results[0]["first"], results[0]["count"]
    for name, _, dtype in PLANES:
        if name not in results[0]:
            continue
        acc = np.zeros(out["count"], dtype=np.uint64)
        for r in results:
            if name not in r or len(r[name]) != len(acc) or (r["first"], r["count"]) != (out["first"], out["count"]):
                raise ValueError("merge: results of different configs")
            acc += np.ascontiguousarray(r[name]).view(np.uint64)  # modulo 2**64
        out[name] = acc.view(dtype)
    return out
