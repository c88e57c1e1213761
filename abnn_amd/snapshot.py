"""Device-side snapshots (abnn.h ``abnn_snapshot_*``) on the host side.

Capture, restore and the diff run in the HIP library (csrc/capi.hip,
csrc/snapshot.hip).  This module holds the :class:`Snapshot` object over them
and what needs no GPU: the diff's config, the decoding of a result into a
dict, the numpy restatement of the rule over interchange records
(:func:`reference`: the test reference, which never calls the library) and the
merge of several results (:func:`merge`: shards).  Every word is an integer
sum or maximum and every float operation a single float32 operation, so
:func:`reference` equals the device bit for bit.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import DIFF_HEADER_WORDS, DIFF_MAX_BINS, SNAP_RECORDS, SNAP_STATE, DiffConfig, SnapshotInfo, call

F32 = np.float32
TOMB = np.uint32(0xFFFFFFFF)
# words 0 .. 18 and 21 by name; 19 (net) is an int64, 20 (abs) a u64, 22 the float max_abs
_COUNT_KEYS = ("n_now", "n_then", "compared", "born", "gone", "dead_both", "killed", "revived", "rewired", "paired",
               "selected", "same", "changed", "up", "down", "zero", "nan", "under", "over")
PARTS = {"records": SNAP_RECORDS, "state": SNAP_STATE}


def config(bins: int, lo: float, hi: float, src: Optional[Sequence[int]] = None,
           dst: Optional[Sequence[int]] = None) -> DiffConfig:
    """``bins`` bins over d = w_now - w_then in [lo, hi); ``src`` / ``dst`` are
    (first, count) pairs, None (or count 0) = any."""
    s = (0, 0) if src is None else (int(src[0]), int(src[1]))
    d = (0, 0) if dst is None else (int(dst[0]), int(dst[1]))
    return DiffConfig(float(lo), float(hi), int(bins), s[0], s[1], d[0], d[1], 0)


def _scale(cfg: DiffConfig) -> np.float32:
    """(float)bins / (hi - lo) in float32, or ValueError for what abnn_snapshot_diff_words refuses."""
    lo, hi = F32(cfg.lo), F32(cfg.hi)
    if not 1 <= cfg.bins <= DIFF_MAX_BINS or cfg.reserved != 0:
        raise ValueError("diff: bins must be 1..4096 and reserved 0")
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError("diff: lo < hi, both finite")
    with np.errstate(over="ignore", divide="ignore"):
        span = hi - lo
        scale = F32(cfg.bins) / span
    if not (np.isfinite(span) and np.isfinite(scale)):
        raise ValueError("diff: hi - lo and bins / (hi - lo) must be finite in float32")
    return scale


def n_words(cfg: DiffConfig) -> int:
    """abnn_snapshot_diff_words: 24 + bins, or 0 for an invalid config."""
    try:
        _scale(cfg)
    except ValueError:
        return 0
    return DIFF_HEADER_WORDS + int(cfg.bins)


def edges(cfg: DiffConfig) -> np.ndarray:
    """bins + 1 nominal bin edges (float64); the bin of a d is defined by the
    float32 formula of abnn.h, which may differ from these by a rounding."""
    return float(cfg.lo) + (float(cfg.hi) - float(cfg.lo)) * np.arange(cfg.bins + 1, dtype=np.float64) / cfg.bins


def decode(words: np.ndarray, cfg: DiffConfig) -> dict:
    """A result's u64 words (abnn.h) as a dict: the counts by name, ``net`` and
    ``abs`` in 2**-24 fixed point (int), ``not_summable``, ``max_abs``
    (float32: the largest |d|), ``counts`` (np.uint64) and ``edges``."""
    w = np.asarray(words, dtype=np.uint64)
    assert w.shape == (DIFF_HEADER_WORDS + cfg.bins,), w.shape
    d = {k: int(w[i]) for i, k in enumerate(_COUNT_KEYS)}
    d["net"] = int(w[19:20].view(np.int64)[0])
    d["abs"] = int(w[20])
    d["not_summable"] = int(w[21])
    d["max_abs"] = np.array([int(w[22]) & 0xFFFFFFFF], dtype=np.uint32).view(F32)[0]
    d["counts"] = w[DIFF_HEADER_WORDS:].copy()
    d["edges"] = edges(cfg)
    return d


def to_words(d: dict) -> np.ndarray:
    """The inverse of :func:`decode`: the result's u64 words."""
    head = np.zeros(DIFF_HEADER_WORDS, dtype=np.uint64)
    for i, k in enumerate(_COUNT_KEYS):
        head[i] = d[k]
    head[19] = int(d["net"]) & 0xFFFFFFFFFFFFFFFF
    head[20] = d["abs"]
    head[21] = d["not_summable"]
    head[22] = int(np.array([d["max_abs"]], dtype=F32).view(np.uint32)[0])
    return np.concatenate([head, np.asarray(d["counts"], dtype=np.uint64)])


def reference(then: np.ndarray, now: np.ndarray, cfg: DiffConfig) -> dict:
    """The diff of interchange records ``then`` and ``now`` (fields src, dst,
    w) in numpy, by the rule of abnn.h."""
    scale = _scale(cfg)
    lo, hi, bins = F32(cfg.lo), F32(cfg.hi), int(cfg.bins)
    n_then, n_now = len(then), len(now)
    c = min(n_then, n_now)
    a, b = then[:c], now[:c]
    sa, da, sb, db = (x.astype(np.uint32) for x in (a["src"], a["dst"], b["src"], b["dst"]))
    wa = np.ascontiguousarray(a["w"], dtype=F32)
    wb = np.ascontiguousarray(b["w"], dtype=F32)
    ta, tb = da == TOMB, db == TOMB
    live = ~ta & ~tb
    rewired = live & ((sa != sb) | (da != db))
    paired = live & ~rewired
    sel = paired.copy()
    for x, first, count in ((sb, cfg.src_first, cfg.src_count), (db, cfg.dst_first, cfg.dst_count)):
        if count:
            sel &= (x.astype(np.int64) >= first) & (x.astype(np.int64) < first + count)
    same = sel & (wa.view(np.uint32) == wb.view(np.uint32))
    changed = sel & ~same
    va, vb = wa[changed], wb[changed]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        d = vb - va
        oka, okb = np.abs(va) < F32(128.0), np.abs(vb) < F32(128.0)
        ok = oka & okb
        q = (np.trunc(vb[ok] * F32(16777216.0)).astype(np.int64) -
             np.trunc(va[ok] * F32(16777216.0)).astype(np.int64))
    is_nan = d != d
    v = d[~is_nan]
    under, over = v < lo, v >= hi
    mid = v[~under & ~over]
    with np.errstate(under="ignore"):
        idx = np.minimum(((mid - lo) * scale).astype(np.uint32), np.uint32(bins - 1))
    out = {"n_now": n_now, "n_then": n_then, "compared": c, "born": n_now - c, "gone": n_then - c,
           "dead_both": int((ta & tb).sum()), "killed": int((~ta & tb).sum()), "revived": int((ta & ~tb).sum()),
           "rewired": int(rewired.sum()), "paired": int(paired.sum()), "selected": int(sel.sum()),
           "same": int(same.sum()), "changed": int(changed.sum()), "up": int((v > 0).sum()),
           "down": int((v < 0).sum()), "zero": int((v == 0).sum()), "nan": int(is_nan.sum()),
           "under": int(under.sum()), "over": int(over.sum())}
    net = int(q.sum(dtype=np.int64)) if len(q) else 0
    out["net"] = net
    out["abs"] = int(np.abs(q).sum(dtype=np.uint64)) if len(q) else 0
    out["not_summable"] = int((~ok).sum())
    ad = np.abs(v).view(np.uint32)
    out["max_abs"] = np.array([int(ad.max()) if len(ad) else 0], dtype=np.uint32).view(F32)[0]
    out["counts"] = np.bincount(idx, minlength=bins).astype(np.uint64)
    out["edges"] = edges(cfg)
    return out


def merge(results: Iterable[dict]) -> dict:
    """The diff of the union of disjoint record sets (shards) from their diffs
    under one config: every word adds (net modulo 2**64), max_abs takes the
    maximum."""
    results = list(results)
    if not results:
        raise ValueError("merge: no results")
    out = {k: sum(int(r[k]) for r in results) for k in _COUNT_KEYS + ("abs", "not_summable")}
    net = sum(int(r["net"]) for r in results) & 0xFFFFFFFFFFFFFFFF
    out["net"] = net - (1 << 64) if net >> 63 else net
    out["max_abs"] = max((r["max_abs"] for r in results), key=lambda x: int(np.array([x], dtype=F32).view(np.uint32)[0]))
    counts = np.zeros_like(np.asarray(results[0]["counts"], dtype=np.uint64))
    for r in results:
        if len(r["counts"]) != len(counts):
            raise ValueError("merge: results of different configs")
        counts += np.asarray(r["counts"], dtype=np.uint64)
    out["counts"] = counts
    out["edges"] = np.array(results[0]["edges"], copy=True)
    return out


def _stream_ptr(stream) -> Optional[int]:
    if stream is None:
        return None
    if isinstance(stream, int):
        return stream
    return int(getattr(stream, "cuda_stream"))  # torch.cuda.Stream


class Snapshot:
    """A device-side copy of one :class:`abnn_amd.Brain`'s state
    (abnn_snapshot_*): capture it, roll the brain back to it, diff the
    brain's records (or another snapshot's) against it.  Close it before its
    brain."""

    def __init__(self, brain):
        self._brain = brain
        h = C.c_void_p()
        call("abnn_snapshot_create", brain._h, C.byref(h))
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            call("abnn_snapshot_destroy", self._h)
        self._h = None

    def __del__(self):
        try:
            # the brain frees the device; a snapshot that outlived it has nothing left to free safely
            if getattr(self._brain, "_h", None) is not None:
                self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def capture(self, stream=None) -> None:
        """Enqueue a capture on ``stream`` (device-to-device copies in stream
        order; nothing synchronises).  A second capture overwrites the first."""
        call("abnn_snapshot_capture_enqueue", self._brain._h, self._h, _stream_ptr(stream))

    def restore(self, what=("records", "state")) -> None:
        """Roll the brain back (synchronous): ``what`` names the parts,
        "records" (the records and n_syn) and / or "state" (the timestamps,
        the scalars, the inject_inputs RNG, the grown records)."""
        if isinstance(what, str):
            what = (what,)
        bits = 0
        for k in what:
            bits |= PARTS[k]
        call("abnn_snapshot_restore", self._brain._h, self._h, bits)

    def info(self) -> dict:
        """captures, n_syn, clock and pass_index at the last capture, bytes (host view, no synchronise)."""
        i = SnapshotInfo()
        call("abnn_snapshot_get_info", self._h, C.byref(i))
        return {"captures": int(i.captures), "n_syn": int(i.n_syn), "clock": int(i.scalars.clock),
                "pass_index": int(i.scalars.pass_index), "bytes": int(i.bytes)}

    def diff(self, bins: int, lo: float, hi: float, src=None, dst=None, now: Optional["Snapshot"] = None) -> dict:
        """What changed since this snapshot (abnn_snapshot_diff): this
        snapshot's records are ``then``; ``now`` is another snapshot of the
        same brain, or None = the brain's records.  ``bins`` bins over
        d = w_now - w_then in [lo, hi); ``src`` / ``dst`` are (first, count)
        neuron ranges.  Returns :func:`decode`'s dict."""
        cfg = config(bins, lo, hi, src, dst)
        words = int(_lib.load().abnn_snapshot_diff_words(C.byref(cfg)))
        out = np.zeros(max(words, 1), dtype=np.uint64)
        call("abnn_snapshot_diff", self._brain._h, self._h, None if now is None else now._h, C.byref(cfg),
             out.ctypes.data, words)  # an invalid config fails here
        return decode(out, cfg)

    def diff_enqueue(self, cfg: DiffConfig, out_ptr: int, stream=None, now: Optional["Snapshot"] = None) -> None:
        """Enqueue a diff into device memory at ``out_ptr``
        (abnn_snapshot_diff_words(cfg) u64) on ``stream``; nothing
        synchronises.  Decode with :func:`decode`."""
        call("abnn_snapshot_diff_enqueue", self._brain._h, self._h, None if now is None else now._h, C.byref(cfg),
             int(out_ptr), _stream_ptr(stream))
