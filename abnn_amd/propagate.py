"""Signal propagation (abnn.h ``abnn_propagate_*``) on the host side.

The pass itself runs in the HIP library (csrc/propagate.hip); this module holds
what needs no GPU: the config, the decoding of a result into a dict, the numpy
restatement of the rule over interchange records (:func:`reference`,
:func:`rescale_reference`, :func:`iterate_reference`: the test reference, and
usable for small brains), the library's own host rule (:func:`host`,
:func:`rescale_host`), the sum of the shards' results (:func:`merge`) and the
reading of an iteration's trace (:func:`branching`).  Every word is an integer,
so :func:`reference` equals the device word for word.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import (PROP_FIRE_P, PROP_HEADER_WORDS, PROP_MAX_STEPS, PROP_REVERSE, PROP_TRACE_WORDS, PROP_WEIGHT,
                   PropagateConfig)

F32 = np.float32
U32 = np.uint32
I64 = np.int64
U64 = np.uint64
ONE = 1 << 30        # the helpers' fixed point of x: to_fixed(1.0)
Y_FRAC_BITS = 8      # y carries this many fractional bits more than x
NARROW_MAX = 4096    # csrc/propagate.h kPropNarrowMax: longer out-ranges take the atomics path
SPARSE_DIV = 4       # csrc/propagate.h kPropSparseDiv: forward, sparse when nnz * SPARSE_DIV <= N_NRN
# csrc/propagate.h kPropFoldWords / kPropFoldMaxNnz: the sparse instance tests records against an LDS fold of the
# non-zero map (FOLD_WORDS u32) when nnz is at most FOLD_MAX_NNZ or the whole map fits, and against the map otherwise
FOLD_WORDS = 4096
FOLD_MAX_NNZ = 32 * FOLD_WORDS // 2
_COUNT_KEYS = ("records", "tombstones", "followed", "skipped", "nnz", "sum_abs_x")  # words 0..5
_TRACE_KEYS = ("nnz", "sum_abs_x", "sum_abs_y", "max_abs_y", "e", "followed", "skipped")  # a row's words 0..6
_ALL = PROP_REVERSE | PROP_FIRE_P | PROP_WEIGHT


def config(inputs: Optional[Sequence[int]] = None, outputs: Optional[Sequence[int]] = None, reverse: bool = False,
           fire_p: bool = False, weights: Optional[Sequence[float]] = None) -> PropagateConfig:
    """``inputs`` / ``outputs`` are the (first, count) neuron ranges x is read
    from and y is summed over (None: every neuron); ``reverse`` is the
    transpose (kin = dst, kout = src); ``fire_p`` takes (w*w)*base_scale for
    the coefficient, not w; ``weights`` = (w_lo, w_hi) follows only records
    with w_lo <= w < w_hi (inf allowed)."""
    i = (0, 0) if inputs is None else (int(inputs[0]), int(inputs[1]))
    o = (0, 0) if outputs is None else (int(outputs[0]), int(outputs[1]))
    lo, hi = (0.0, 0.0) if weights is None else (float(weights[0]), float(weights[1]))
    flags = (PROP_REVERSE if reverse else 0) | (PROP_FIRE_P if fire_p else 0) | (PROP_WEIGHT if weights is not None else 0)
    return PropagateConfig(i[0], i[1], o[0], o[1], flags, lo, hi)  # reserved: zeros


def _bits(x: float) -> int:
    return int(np.array([x], dtype=F32).view(U32)[0])


def config_ok(cfg: Optional[PropagateConfig], n_nrn: int) -> bool:
    """The checks of abnn_propagate_words."""
    n_nrn = int(n_nrn)
    if cfg is None or not 0 < n_nrn < 1 << 32 or cfg.flags & ~_ALL or any(cfg.reserved):
        return False
    for first, count in ((cfg.in_first, cfg.in_count), (cfg.out_first, cfg.out_count)):
        if (count == 0 and first != 0) or first + count > n_nrn:
            return False
    if cfg.flags & PROP_WEIGHT:
        if not F32(cfg.w_lo) < F32(cfg.w_hi):  # false for a NaN bound
            return False
    elif _bits(cfg.w_lo) or _bits(cfg.w_hi):
        return False
    return True


def ranges(cfg: PropagateConfig, n_nrn: int) -> tuple[int, int, int, int]:
    """(in_first, in_count, out_first, out_count) with a count of 0 resolved to every neuron."""
    n_nrn = int(n_nrn)
    return (int(cfg.in_first) if cfg.in_count else 0, int(cfg.in_count) or n_nrn,
            int(cfg.out_first) if cfg.out_count else 0, int(cfg.out_count) or n_nrn)


def n_words(cfg: PropagateConfig, n_nrn: int) -> int:
    """abnn_propagate_words: 8 + the neurons of the out-range, or 0 for an invalid config."""
    if not config_ok(cfg, n_nrn):
        return 0
    return PROP_HEADER_WORDS + ranges(cfg, n_nrn)[3]


def to_fixed(a, one: int = ONE) -> np.ndarray:
    """Real activities as the int32 fixed point of x: round(a * one), saturated."""
    v = np.rint(np.asarray(a, dtype=np.float64) * float(one))
    return np.clip(v, -(1 << 31), (1 << 31) - 1).astype(np.int32)


def from_fixed(v, one: int = ONE, frac_bits: int = 0) -> np.ndarray:
    """The inverse of :func:`to_fixed`; a y plane takes ``frac_bits=Y_FRAC_BITS``."""
    return np.asarray(v).astype(np.float64) / (float(one) * float(1 << frac_bits))


def _abs_u64(y: np.ndarray) -> np.ndarray:
    """|y| of int64 words as uint64: INT64_MIN counts as 2**63."""
    u = np.ascontiguousarray(y).view(U64)
    return np.where(u >> U64(63), U64(0) - u, u)


def reference(syn: np.ndarray, cfg: PropagateConfig, n_nrn: int, x: np.ndarray, base_scale: float = 0.0) -> dict:
    """The rule of abnn.h over interchange records ``syn`` (fields src, dst, w)
    in numpy: the header counts and ``y`` (np.int64, the out-range)."""
    if not config_ok(cfg, n_nrn):
        raise ValueError("propagate: invalid config")
    x = np.ascontiguousarray(x, dtype=np.int32)
    if x.shape != (int(n_nrn),):
        raise ValueError("propagate: x must hold N_NRN entries")
    i0, ic, o0, oc = ranges(cfg, n_nrn)
    src, dst, w = syn["src"].astype(U32), syn["dst"].astype(U32), syn["w"].astype(F32)
    live = dst != U32(0xFFFFFFFF)
    kin, kout = (dst, src) if cfg.flags & PROP_REVERSE else (src, dst)
    m = live & ((kin - U32(i0)) < U32(ic)) & ((kout - U32(o0)) < U32(oc))  # u32 arithmetic wraps
    if cfg.flags & PROP_WEIGHT:
        with np.errstate(invalid="ignore"):
            m &= (w >= F32(cfg.w_lo)) & (w < F32(cfg.w_hi))  # false for NaN
    idx = np.flatnonzero(m)
    xv = x[kin[idx].astype(I64)]
    idx, xv = idx[xv != 0], xv[xv != 0]
    c = w[idx]
    with np.errstate(over="ignore", invalid="ignore"):
        if cfg.flags & PROP_FIRE_P:
            c = (c * c) * F32(base_scale)  # two fp32 operations
        summable = np.abs(c) < F32(128.0)  # false for NaN and +-inf
    q = (np.where(summable, c, F32(0)) * F32(16777216.0)).astype(np.int32)  # exact product, truncation toward zero
    term = (q.astype(I64) * xv.astype(I64)) >> I64(16)
    y = np.zeros(oc, dtype=U64)
    keep = summable
    np.add.at(y, (kout[idx][keep] - U32(o0)).astype(I64), term[keep].view(U64))  # modulo 2**64
    xin = x[i0:i0 + ic].astype(I64)
    return {"records": int(len(syn)), "tombstones": int((~live).sum()), "followed": int(len(idx)),
            "skipped": int((~summable).sum()), "nnz": int((xin != 0).sum()), "sum_abs_x": int(np.abs(xin).sum()),
            "y": y.view(I64)}


def rescale_reference(d: dict, cfg: PropagateConfig, n_nrn: int, x: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """The rescale of a result ``d`` into a copy of ``x`` over the out-range:
    (the next x, the trace row of 8 u64)."""
    _, _, o0, oc = ranges(cfg, n_nrn)
    y = np.ascontiguousarray(d["y"], dtype=I64)
    mag = _abs_u64(y)
    mx = int(mag.max()) if len(mag) else 0
    total = int(mag.sum(dtype=U64))  # modulo 2**64
    e = 30 - mx.bit_length() if mx else 0
    if e >= 0:
        scaled = (y.view(U64) << U64(e)).view(I64)
    else:
        scaled = y >> I64(-e)  # arithmetic
    out = np.array(x, dtype=np.int32, copy=True)
    out[o0:o0 + oc] = (scaled.view(U64) & U64(0xFFFFFFFF)).astype(U32).view(np.int32)
    row = np.array([d["nnz"], d["sum_abs_x"], total, mx, e % (1 << 64), d["followed"], d["skipped"], 0], dtype=U64)
    return out, row


def iterate_reference(syn: np.ndarray, cfg: PropagateConfig, n_nrn: int, x: np.ndarray, steps: int,
                      base_scale: float = 0.0) -> tuple[np.ndarray, np.ndarray]:
    """``steps`` times propagate and rescale in numpy: (the last x, the trace of steps x 8 u64)."""
    if (cfg.in_first, cfg.in_count) != (cfg.out_first, cfg.out_count):
        raise ValueError("propagate: iterate needs the in-range and the out-range to be the same")
    if not 1 <= int(steps) <= PROP_MAX_STEPS:
        raise ValueError("propagate: steps must be 1 .. %d" % PROP_MAX_STEPS)
    x = np.array(x, dtype=np.int32, copy=True)
    trace = np.zeros((int(steps), PROP_TRACE_WORDS), dtype=U64)
    for k in range(int(steps)):
        x, trace[k] = rescale_reference(reference(syn, cfg, n_nrn, x, base_scale), cfg, n_nrn, x)
    return x, trace


def host(syn: np.ndarray, cfg: PropagateConfig, n_nrn: int, x: np.ndarray, base_scale: float = 0.0) -> np.ndarray:
    """abnn_propagate_host: the library's host rule over interchange records
    (the SYN_DTYPE of abnn_amd.brain); the result's u64 words."""
    from .brain import SYN_DTYPE

    syn = np.ascontiguousarray(syn, dtype=SYN_DTYPE)
    x = np.ascontiguousarray(x, dtype=np.int32)
    words = n_words(cfg, n_nrn)
    if not words or x.shape != (int(n_nrn),):
        raise ValueError("propagate: invalid config or x")
    out = np.zeros(words, dtype=U64)
    _lib.call("abnn_propagate_host", C.byref(cfg), int(n_nrn), float(base_scale), syn.ctypes.data, len(syn),
              x.ctypes.data, out.ctypes.data)
    return out


def rescale_host(words: np.ndarray, cfg: PropagateConfig, n_nrn: int, x: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """abnn_propagate_rescale_host: (the next x, the trace row)."""
    w = np.ascontiguousarray(words, dtype=U64)
    out = np.array(x, dtype=np.int32, copy=True)
    if w.shape != (n_words(cfg, n_nrn),) or not len(w) or out.shape != (int(n_nrn),):
        raise ValueError("propagate: invalid config, words or x")
    row = np.zeros(PROP_TRACE_WORDS, dtype=U64)
    _lib.call("abnn_propagate_rescale_host", C.byref(cfg), int(n_nrn), w.ctypes.data, out.ctypes.data, row.ctypes.data)
    return out, row


def decode(words: np.ndarray, cfg: PropagateConfig, n_nrn: int) -> dict:
    """A result's u64 words (abnn.h) as a dict: the header counts and ``y`` (np.int64)."""
    w = np.ascontiguousarray(words, dtype=U64)
    assert n_words(cfg, n_nrn) and w.shape == (n_words(cfg, n_nrn),), (w.shape, n_nrn)
    d = {k: int(w[i]) for i, k in enumerate(_COUNT_KEYS)}
    d["y"] = w[PROP_HEADER_WORDS:].view(I64).copy()
    return d


def to_words(d: dict) -> np.ndarray:
    """The inverse of :func:`decode`."""
    head = np.array([d[k] for k in _COUNT_KEYS] + [0, 0], dtype=U64)
    return np.concatenate([head, np.ascontiguousarray(d["y"], dtype=I64).view(U64)])


def merge(parts: Iterable[dict]) -> dict:
    """The sum of the shards' results: the record counts and y add (y modulo
    2**64); nnz and sum_abs_x describe the one x every shard read and must
    agree.  The rescale follows the merge."""
    parts = list(parts)
    if not parts:
        raise ValueError("merge: no results")
    out = {k: 0 for k in _COUNT_KEYS}
    y = np.zeros(len(parts[0]["y"]), dtype=U64)
    for p in parts:
        if len(p["y"]) != len(y) or (p["nnz"], p["sum_abs_x"]) != (parts[0]["nnz"], parts[0]["sum_abs_x"]):
            raise ValueError("merge: results of different ranges or different x")
        for k in _COUNT_KEYS[:4]:
            out[k] = (out[k] + p[k]) % (1 << 64)
        y += np.ascontiguousarray(p["y"], dtype=I64).view(U64)
    out["nnz"], out["sum_abs_x"] = parts[0]["nnz"], parts[0]["sum_abs_x"]
    out["y"] = y.view(I64)
    return out


def branching(trace: np.ndarray) -> dict:
    """An iteration's trace (steps x 8 u64) as a dict: per step ``estimates``
    = (sum |y| / 256) / sum |x| (0 where x was zero), the row's words by name
    (``e`` as int64), and ``ratio``, the last step's estimate: for non-negative
    coefficients and start the spectral radius of the operator on the range,
    with fire_p the branching ratio."""
    t = np.ascontiguousarray(trace, dtype=U64).reshape(-1, PROP_TRACE_WORDS)
    d = {k: t[:, i].copy() for i, k in enumerate(_TRACE_KEYS)}
    d["e"] = d["e"].view(I64)
    sx, sy = d["sum_abs_x"].astype(np.float64), d["sum_abs_y"].astype(np.float64)
    d["estimates"] = np.divide(sy / float(1 << Y_FRAC_BITS), sx, out=np.zeros_like(sx), where=sx > 0)
    d["ratio"] = float(d["estimates"][-1]) if len(t) else 0.0
    return d
