"""Spike correlograms (abnn.h ``abnn_corr_*``) on the host side.

The correlogram itself runs in the HIP library (csrc/corr.hip); this module
holds what needs no GPU: the config, the decoding of a result into a dict, the
merge of the shards' results and the numpy restatement of the rule over a pass
table, a raster and interchange records (:func:`reference`: the test
reference, and usable for small brains).  It shares no code with the C host
rule (csrc/corr.h): dense per-neuron row-count matrices instead of lists.
Every word is an integer sum, so :func:`reference` equals the device word for
word.
"""
from __future__ import annotations

from typing import Iterable, Optional, Sequence

import numpy as np

from ._lib import (CORR_HEADER_WORDS, CORR_MAX_LAG, CORR_MAX_PAIR_WORDS, CORR_PAIRS, CORR_POP, CORR_SYNAPSES,
                   CORR_WEIGHT, CorrConfig)

F32 = np.float32
U32 = np.uint32
U64 = np.uint64
MODES = {"pop": CORR_POP, "pairs": CORR_PAIRS, "synapses": CORR_SYNAPSES}
KEYS = ("rows", "entries", "in_a", "in_b", "total", "followed", "coupled", "recorded")  # words 0..7


def config(mode, a: Optional[Sequence[int]] = None, b: Optional[Sequence[int]] = None, max_lag: int = 16,
           rows: Optional[Sequence[int]] = None, weights: Optional[Sequence[float]] = None) -> CorrConfig:
    """``mode`` is "pop", "pairs" or "synapses" (or the constant); ``a`` / ``b``
    = (first, count) of the pre / post population or None for every neuron;
    ``rows`` = (first, count) of the table rows or None for all (count 0 =
    through the last); ``weights`` = (w_lo, w_hi) follows only records with
    w_lo <= w < w_hi (SYNAPSES).  Nothing is checked here: abnn_corr_words does."""
    af, ac = (0, 0) if a is None else (int(a[0]), int(a[1]))
    bf, bc = (0, 0) if b is None else (int(b[0]), int(b[1]))
    rf, rc = (0, 0) if rows is None else (int(rows[0]), int(rows[1]))
    lo, hi = (0.0, 0.0) if weights is None else (float(weights[0]), float(weights[1]))
    m = MODES[mode] if isinstance(mode, str) else int(mode)
    return CorrConfig(af, ac, bf, bc, rf, rc, int(max_lag), m, CORR_WEIGHT if weights is not None else 0, lo, hi)


def _bits(x: float) -> int:
    return int(np.array([x], dtype=F32).view(U32)[0])


def plane_words(cfg: Optional[CorrConfig]) -> int:
    """The plane's u64 words, or 0 for an invalid config (the checks of abnn_corr_words)."""
    if cfg is None or cfg.mode not in (CORR_POP, CORR_PAIRS, CORR_SYNAPSES) or cfg.flags & ~CORR_WEIGHT:
        return 0
    if cfg.max_lag > CORR_MAX_LAG or any(cfg.reserved):
        return 0
    if cfg.a_first + cfg.a_count > 1 << 32 or cfg.b_first + cfg.b_count > 1 << 32:
        return 0
    if cfg.flags & CORR_WEIGHT:
        if not F32(cfg.w_lo) < F32(cfg.w_hi):  # false for a NaN bound
            return 0
    elif _bits(cfg.w_lo) or _bits(cfg.w_hi):
        return 0
    nb = 2 * int(cfg.max_lag) + 1
    if cfg.mode != CORR_PAIRS:
        return nb
    if cfg.a_count == 0 or cfg.b_count == 0 or cfg.a_count * cfg.b_count * nb > CORR_MAX_PAIR_WORDS:
        return 0
    return cfg.a_count * cfg.b_count * nb


def n_words(cfg: Optional[CorrConfig]) -> int:
    """abnn_corr_words: 8 + the plane, or 0 for an invalid config."""
    p = plane_words(cfg)
    return CORR_HEADER_WORDS + p if p else 0


def decode(out: np.ndarray, cfg: CorrConfig) -> dict:
    """A result's u64 words as a dict: the header under KEYS, ``lags`` (-L..L)
    and ``plane`` (np.uint64): (2L+1,) or, for PAIRS, (a_count, b_count, 2L+1)."""
    w = np.ascontiguousarray(out, dtype=U64)
    assert n_words(cfg) and w.shape == (n_words(cfg),), w.shape
    d = {k: int(w[i]) for i, k in enumerate(KEYS)}
    L = int(cfg.max_lag)
    d["lags"] = np.arange(-L, L + 1, dtype=np.int64)
    plane = w[CORR_HEADER_WORDS:].copy()
    d["plane"] = plane.reshape(cfg.a_count, cfg.b_count, 2 * L + 1) if cfg.mode == CORR_PAIRS else plane
    return d


def to_words(d: dict) -> np.ndarray:
    """The inverse of :func:`decode`."""
    head = np.array([d[k] for k in KEYS], dtype=U64)
    return np.concatenate([head, np.ascontiguousarray(d["plane"], dtype=U64).reshape(-1)])


def merge(results: Iterable[dict]) -> dict:
    """The ranks' SYNAPSES results as the whole graph's: words 4..6 and the
    plane summed; the rest (the same on every rank) from the first."""
    results = list(results)
    if not results:
        raise ValueError("merge: no results")
    out = dict(results[0])
    out["plane"] = results[0]["plane"].copy()
    for r in results[1:]:
        if r["plane"].shape != out["plane"].shape:
            raise ValueError("merge: planes of different sizes")
        out["plane"] = out["plane"] + r["plane"]
        for k in ("total", "followed", "coupled"):
            out[k] = (out[k] + r[k]) & 0xFFFFFFFFFFFFFFFF
    return out


def _in(ids: np.ndarray, first: int, count: int, n_nrn: int) -> np.ndarray:
    ok = ids.astype(np.int64) < n_nrn
    return ok & (ids.astype(U32) - U32(first) < U32(count)) if count else ok


def reference(cfg: CorrConfig, n_nrn: int, passes: np.ndarray, raster: np.ndarray,
              records: Optional[np.ndarray] = None) -> dict:
    """The rule of abnn.h in numpy over a pass table (spikes.SPIKE_PASS_DTYPE),
    its raster and, for SYNAPSES, interchange records (fields src, dst, w); K =
    len(passes) and the raster's length is its capacity.  Returns what
    :func:`decode` returns."""
    if not n_words(cfg):
        raise ValueError("corr: invalid config")
    n_nrn, L, K = int(n_nrn), int(cfg.max_lag), len(passes)
    if max(cfg.a_first + cfg.a_count, cfg.b_first + cfg.b_count) > n_nrn:
        raise ValueError("corr: a range ends above N_NRN")
    raster = np.asarray(raster, dtype=U32)
    lo = min(int(cfg.row_first), K)
    hi = K if cfg.row_count == 0 else min(K, lo + int(cfg.row_count))
    R = hi - lo
    # CA[x, r] / CB[y, r]: the entries of neuron x in window row r, by population
    CA = np.zeros((n_nrn, R), dtype=np.int64)
    CB = np.zeros((n_nrn, R), dtype=np.int64)
    entries = 0
    for r in range(R):
        off = min(int(passes[lo + r]["offset"]), len(raster))
        ids = raster[off:off + min(int(passes[lo + r]["count"]), len(raster) - off)]
        entries += len(ids)
        np.add.at(CA[:, r], ids[_in(ids, cfg.a_first, cfg.a_count, n_nrn)].astype(np.int64), 1)
        np.add.at(CB[:, r], ids[_in(ids, cfg.b_first, cfg.b_count, n_nrn)].astype(np.int64), 1)
    d = dict.fromkeys(KEYS, 0)
    d.update(rows=R, entries=entries, in_a=int(CA.sum()), in_b=int(CB.sum()), recorded=K)
    d["lags"] = np.arange(-L, L + 1, dtype=np.int64)

    def shifted(l):  # (rows of A, rows of B) for lag l: q = p + l, both in the window
        n = R - abs(l)
        return (slice(0, n), slice(l, l + n)) if l >= 0 else (slice(-l, -l + n), slice(0, n))

    lags = [l for l in range(-L, L + 1) if abs(l) < R]
    if cfg.mode == CORR_POP:
        plane = np.zeros(2 * L + 1, dtype=np.int64)
        ta, tb = CA.sum(axis=0), CB.sum(axis=0)
        for l in lags:
            pa, pb = shifted(l)
            plane[l + L] = int((ta[pa] * tb[pb]).sum())
    elif cfg.mode == CORR_PAIRS:
        A = CA[cfg.a_first:cfg.a_first + cfg.a_count]
        B = CB[cfg.b_first:cfg.b_first + cfg.b_count]
        plane = np.zeros((cfg.a_count, cfg.b_count, 2 * L + 1), dtype=np.int64)
        for l in lags:
            pa, pb = shifted(l)
            plane[:, :, l + L] = A[:, pa] @ B[:, pb].T
    else:
        if records is None:
            records = np.zeros(0, dtype=[("src", "<u4"), ("dst", "<u4"), ("w", "<f4"), ("pad", "<u4")])
        src, dst = records["src"].astype(np.int64), records["dst"].astype(np.int64)
        m = (dst != 0xFFFFFFFF) & (src < n_nrn) & (dst < n_nrn)
        m &= _in(records["src"], cfg.a_first, cfg.a_count, n_nrn) & _in(records["dst"], cfg.b_first, cfg.b_count, n_nrn)
        if cfg.flags & CORR_WEIGHT:
            w = records["w"].astype(F32)
            with np.errstate(invalid="ignore"):
                m &= (w >= F32(cfg.w_lo)) & (w < F32(cfg.w_hi))  # false for NaN
        s, t = src[m], dst[m]
        plane = np.zeros(2 * L + 1, dtype=np.int64)
        per_record = np.zeros(len(s), dtype=np.int64)
        for l in lags:
            pa, pb = shifted(l)
            v = (CA[s][:, pa] * CB[t][:, pb]).sum(axis=1) if len(s) else per_record
            plane[l + L] = int(v.sum())
            per_record = per_record + v
        d["followed"], d["coupled"] = int(m.sum()), int((per_record > 0).sum())
    d["plane"] = plane.astype(U64)
    d["total"] = int(plane.sum())
    return d
