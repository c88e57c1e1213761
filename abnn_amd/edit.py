"""The synapse edit (abnn.h ``abnn_edit_*``) on the host side.

The edit itself runs in the HIP library (csrc/edit.hip); this module holds what
needs no GPU: the config, the decoding of the 8-word result, the numpy
restatement of the rule over interchange records (:func:`reference`: the test
reference, and usable for small brains), the factors of synaptic scaling
(:func:`factors`) and the sum of the shards' headers (:func:`merge`).  Every
operation of the rule is one uint32 or float32 operation, so :func:`reference`
equals the device bit for bit.
"""
from __future__ import annotations

from typing import Iterable, Optional, Sequence, Tuple, Union

import numpy as np

from . import select as _select
from ._lib import (EDIT_AFFINE, EDIT_ANY, EDIT_CLAMP, EDIT_DRAW, EDIT_HEADER_WORDS, EDIT_KEY, EDIT_KILL,
                   EDIT_SCALE_DST, EDIT_SCALE_SRC, EDIT_SET, EDIT_WEIGHT, EditConfig, SelectConfig)
from .graph import _splitmix64_at, _unit24

F32 = np.float32
U32 = np.uint32
U64 = np.uint64
SYN_DTYPE = _select.SYN_DTYPE
OPS = {"set": EDIT_SET, "affine": EDIT_AFFINE, "scale_dst": EDIT_SCALE_DST, "scale_src": EDIT_SCALE_SRC,
       "draw": EDIT_DRAW, "kill": EDIT_KILL}
KEYS = ("records", "tombstones", "matched", "changed", "killed", "nonfinite")  # words 0..5
NAN_BITS = 0x7FC00000  # csrc/edit.h kEditNaN
_ALL = EDIT_ANY | EDIT_WEIGHT | EDIT_CLAMP
_SCALE = (EDIT_SCALE_DST, EDIT_SCALE_SRC)


def op_code(op: Union[int, str]) -> int:
    if isinstance(op, str):
        if op not in OPS:
            raise ValueError(f"edit: unknown op {op!r}")
        return OPS[op]
    return int(op)


def config(op: Union[int, str], src: Optional[Sequence[int]] = None, dst: Optional[Sequence[int]] = None,
           weights: Optional[Sequence[float]] = None, any: bool = False, a: float = 0.0, b: float = 0.0,
           clamp: Optional[Sequence[float]] = None, seed: int = 0) -> EditConfig:
    """``op``: an EDIT_* value or its name (set, affine, scale_dst, scale_src,
    draw, kill).  ``src`` / ``dst`` / ``weights`` / ``any`` are the select's;
    ``a`` / ``b`` the op's parameters (set: b; affine: w * a + b; draw: uniform
    in [a, b]); ``clamp`` = (c_lo, c_hi) clamps the new value; ``seed``: draw."""
    sf, sc = (0, 0) if src is None else (int(src[0]), int(src[1]))
    df, dc = (0, 0) if dst is None else (int(dst[0]), int(dst[1]))
    lo, hi = (0.0, 0.0) if weights is None else (float(weights[0]), float(weights[1]))
    c_lo, c_hi = (0.0, 0.0) if clamp is None else (float(clamp[0]), float(clamp[1]))
    flags = (EDIT_ANY if any else 0) | (EDIT_WEIGHT if weights is not None else 0) | \
        (EDIT_CLAMP if clamp is not None else 0)
    return EditConfig(sf, sc, df, dc, lo, hi, flags, op_code(op), float(a), float(b), c_lo, c_hi,
                      int(seed) & (2**64 - 1))  # reserved: zeros


def _bits(x: float) -> int:
    return int(np.array([x], dtype=F32).view(U32)[0])


def _select_part(cfg: EditConfig) -> SelectConfig:
    return SelectConfig(cfg.src_first, cfg.src_count, cfg.dst_first, cfg.dst_count, cfg.w_lo, cfg.w_hi,
                        cfg.flags & (EDIT_ANY | EDIT_WEIGHT), 0)


def config_ok(cfg: Optional[EditConfig], n_nrn: Optional[int] = None) -> bool:
    """The checks of abnn_edit_words; with ``n_nrn`` also the handle's (a set
    range ends at or below N_NRN)."""
    if cfg is None or cfg.flags & ~_ALL or cfg.op > EDIT_KILL or any(cfg.reserved):
        return False
    if not _select.config_ok(_select_part(cfg), n_nrn):
        return False
    op, clamp = cfg.op, bool(cfg.flags & EDIT_CLAMP)
    reads_a = op in (EDIT_AFFINE, EDIT_DRAW)
    reads_b = reads_a or op == EDIT_SET
    if np.isnan(cfg.a) if reads_a else _bits(cfg.a):
        return False
    if np.isnan(cfg.b) if reads_b else _bits(cfg.b):
        return False
    if clamp:
        if op == EDIT_KILL or not F32(cfg.c_lo) <= F32(cfg.c_hi):  # false for a NaN bound
            return False
    elif _bits(cfg.c_lo) or _bits(cfg.c_hi):
        return False
    if op == EDIT_DRAW:
        if not (np.isfinite(cfg.a) and np.isfinite(cfg.b) and F32(cfg.a) <= F32(cfg.b)):
            return False
    elif cfg.seed:
        return False
    if cfg.flags & EDIT_ANY and op in _SCALE:
        return False
    return True


def n_words(cfg: EditConfig) -> int:
    """abnn_edit_words: 8, or 0 for an invalid config."""
    return EDIT_HEADER_WORDS if config_ok(cfg) else 0


def plane_range(cfg: EditConfig, n_nrn: int) -> Tuple[int, int]:
    """(first, M) of a SCALE op's plane; (0, 0) for another op."""
    if cfg.op not in _SCALE:
        return 0, 0
    first, count = (cfg.dst_first, cfg.dst_count) if cfg.op == EDIT_SCALE_DST else (cfg.src_first, cfg.src_count)
    return (int(first), int(count)) if count else (0, int(n_nrn))


def decode(words: np.ndarray) -> dict:
    """The 8 u64 words of a result as a dict (KEYS)."""
    w = np.asarray(words, dtype=np.uint64)
    assert w.shape == (EDIT_HEADER_WORDS,), w.shape
    return {k: int(w[i]) for i, k in enumerate(KEYS)}


def reference(syn: np.ndarray, cfg: EditConfig, n_nrn: int, syn_offset: int = 0,
              plane: Optional[np.ndarray] = None) -> Tuple[np.ndarray, dict]:
    """The edit of interchange records ``syn`` in numpy: (the new records, a
    copy; the header as :func:`decode` gives it).  ``plane``: the M float32
    factors of a SCALE op."""
    if not config_ok(cfg, n_nrn):
        raise ValueError("edit: invalid config")
    first, m_plane = plane_range(cfg, n_nrn)
    if (plane is not None) != (cfg.op in _SCALE):
        raise ValueError("edit: a SCALE op needs a plane, every other op none")
    out = np.ascontiguousarray(syn, dtype=SYN_DTYPE).copy()
    m = _select.matches(out, _select_part(cfg))
    at = np.flatnonzero(m)
    head = {"records": int(len(out)), "tombstones": int((out["dst"] == U32(0xFFFFFFFF)).sum()),
            "matched": int(len(at)), "changed": 0, "killed": 0, "nonfinite": 0}
    if cfg.op == EDIT_KILL:
        out["src"][at] = 0xFFFFFFFF
        out["dst"][at] = 0xFFFFFFFF
        out["pad"][at] = 0.0
        head["changed"] = head["killed"] = int(len(at))
        return out, head
    w = out["w"][at].astype(F32)
    old = w.view(U32).copy()
    with np.errstate(all="ignore"):
        if cfg.op == EDIT_SET:
            v = np.full(len(at), F32(cfg.b), dtype=F32)
        elif cfg.op == EDIT_AFFINE:
            t = (w * F32(cfg.a)).astype(F32)
            v = (t + F32(cfg.b)).astype(F32)
        elif cfg.op == EDIT_DRAW:
            u = _unit24(_splitmix64_at((int(cfg.seed) ^ EDIT_KEY) & (2**64 - 1), at.astype(U64) + U64(syn_offset)))
            d = F32(cfg.b) - F32(cfg.a)  # three separate fp32 operations
            t = (u.astype(F32) * d).astype(F32)
            v = (F32(cfg.a) + t).astype(F32)
        else:
            plane = np.ascontiguousarray(plane, dtype=F32)
            if plane.shape != (m_plane,):
                raise ValueError("edit: the plane must hold one float32 per neuron of the SCALE op's range")
            key = out["dst" if cfg.op == EDIT_SCALE_DST else "src"][at].astype(np.int64) - first
            inside = (key >= 0) & (key < m_plane)  # every valid record's key
            v = w.copy()
            v[inside] = (w[inside] * plane[key[inside]]).astype(F32)
            scaled = inside
        if cfg.flags & EDIT_CLAMP:
            c = v.copy()
            c = np.where(c < F32(cfg.c_lo), F32(cfg.c_lo), c).astype(F32)  # a NaN stays a NaN
            c = np.where(c > F32(cfg.c_hi), F32(cfg.c_hi), c).astype(F32)
            v = np.where(scaled, c, v).astype(F32) if cfg.op in _SCALE else c
    v = v.copy()
    computed = scaled if cfg.op in _SCALE else np.ones(len(at), dtype=bool)
    v.view(U32)[np.isnan(v) & computed] = NAN_BITS  # a NaN is stored as the canonical quiet NaN (abnn.h)
    new = v.view(U32)
    head["changed"] = int((new != old).sum())
    head["nonfinite"] = int(((new & U32(0x7F800000)) == U32(0x7F800000)).sum())
    out["w"][at] = v
    return out, head


def factors(strength_words: np.ndarray, target: float, f_lo: float, f_hi: float) -> np.ndarray:
    """abnn_edit_factors_*: float32 factors from the int64 fixed-point words of a
    degree census's strength plane: S = float32(word) * 2**-24 (the conversion
    rounds to nearest even), f = target / S where S > 0, else 1, clamped to
    [f_lo, f_hi]."""
    target, f_lo, f_hi = F32(target), F32(f_lo), F32(f_hi)
    if not (np.isfinite(target) and target > 0 and np.isfinite(f_hi) and F32(0) < f_lo <= f_hi):
        raise ValueError("edit factors: target > 0 finite and 0 < f_lo <= f_hi finite")
    words = np.ascontiguousarray(strength_words).view(np.int64)
    s = (words.astype(F32) * F32(1.0 / 16777216.0)).astype(F32)
    with np.errstate(all="ignore"):
        f = np.where(s > F32(0), (target / s).astype(F32), F32(1.0)).astype(F32)
    f = np.where(f < f_lo, f_lo, f).astype(F32)
    f = np.where(f > f_hi, f_hi, f).astype(F32)
    return f


def merge(headers: Iterable[dict]) -> dict:
    """The header of the edit of the concatenation of the shards' records:
    every word adds."""
    headers = list(headers)
    if not headers:
        raise ValueError("merge: no results")
    return {k: sum(int(h[k]) for h in headers) for k in KEYS}
