"""Test helpers of the spike correlograms: pass tables and rasters made by hand
or at random, random interchange records, and abnn_corr_host as a function."""
import ctypes as C

import numpy as np

SYN = np.dtype([("src", "<u4"), ("dst", "<u4"), ("w", "<f4"), ("pad", "<u4")])
NONE = 0xFFFFFFFF


def table(rows):
    """(passes, raster) of the given per-row id lists, laid end to end."""
    from abnn_amd.spikes import SPIKE_PASS_DTYPE

    passes = np.zeros(len(rows), dtype=SPIKE_PASS_DTYPE)
    at = 0
    for k, r in enumerate(rows):
        passes[k] = (k, k, at, len(r), 0)
        at += len(r)
    raster = np.concatenate([np.asarray(r, dtype=np.uint32) for r in rows]) if at else np.zeros(0, dtype=np.uint32)
    return passes, raster.astype(np.uint32)


def random_rows(rng, n_nrn, n_rows, max_len):
    """Rows of 0 .. max_len ids with repeats (a few hot neurons)."""
    rows = []
    for _ in range(n_rows):
        n = int(rng.integers(0, max_len + 1))
        ids = rng.integers(0, n_nrn, n)
        hot = rng.random(n) < 0.3
        ids[hot] = rng.integers(0, min(4, n_nrn), int(hot.sum()))
        rows.append(ids.astype(np.uint32))
    return rows


def random_records(rng, n_nrn, n, tombstones=0.1):
    rec = np.zeros(n, dtype=SYN)
    rec["src"] = rng.integers(0, n_nrn, n)
    rec["dst"] = rng.integers(0, n_nrn, n)
    rec["w"] = rng.random(n).astype(np.float32)
    dead = rng.random(n) < tombstones
    rec["src"][dead] = NONE
    rec["dst"][dead] = NONE
    return rec


def host(cfg, n_nrn, passes, raster, records=None):
    """abnn_corr_host: the result's u64 words (the buffer is poisoned first)."""
    from abnn_amd import _lib, corr

    lib = _lib.load()
    words = corr.n_words(cfg)
    assert words and words == lib.abnn_corr_words(C.byref(cfg))
    passes, raster = np.ascontiguousarray(passes), np.ascontiguousarray(raster, dtype=np.uint32)
    out = np.full(words, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    rec = None if records is None else np.ascontiguousarray(records)
    st = lib.abnn_corr_host(C.byref(cfg), n_nrn, passes.ctypes.data if len(passes) else None, len(passes),
                            raster.ctypes.data if len(raster) else None, len(raster),
                            rec.ctypes.data if rec is not None and len(rec) else None, 0 if rec is None else len(rec),
                            out.ctypes.data)
    assert st == 0, lib.abnn_last_error()
    return out


def check(got_words, cfg, n_nrn, passes, raster, records=None):
    """Device words against the numpy reference and the C host rule, word for word."""
    from abnn_amd import corr

    want = corr.to_words(corr.reference(cfg, n_nrn, passes, raster, records))
    got = np.asarray(got_words, dtype=np.uint64)
    assert got[:8].tolist() == want[:8].tolist(), (got[:8].tolist(), want[:8].tolist())
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert np.array_equal(host(cfg, n_nrn, passes, raster, records), want)
    return corr.decode(got, cfg)
