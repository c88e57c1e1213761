"""Test helpers for neuron ids above 2^18 (plain numpy, no GPU).

The blocked pre-spike filter folds bitmap word j = n >> 5 onto block
(j ^ t) mod 8192 with t = 0x9E5 * (j >> 13) and rotates its high image by
t mod 32 (kernels.hip filter_t / filter_set, raw.hip raw_t; engine.h src_code
is the same arithmetic stored per record).  Below 2^18 neurons t is 0: nothing
folds, nothing rotates, and the decoded jh of code_src is always 0.  This
module holds

* the one Python restatement of that arithmetic (`filter_slot`, and the stored
  code `_src_code` / `_code_src` built on it),
* a numpy model of the filter (`filter_model` / `passes_filter`) and of the
  second-level Bloom filter (`f2_model` / `passes_f2`),
* `high_id_graph`: a 1M-record graph that makes every id class n >> 18 carry
  recent neurons, pre-gated records and crafted false positives,
* the debug-bitmap helpers shared by the parity tests.
"""
from __future__ import annotations

import functools

import numpy as np

FILTER_BLOCKS = 8192  # engine.h kCodeFilterWords, raw.hip kRawFB
F2_WORDS = 2048       # engine.h kF2Words
WINDOW_PRE = 5        # default abnn_params.window_pre
CLASS_LOG2 = 18       # ids of one n >> 18 share t


# ---- the filter arithmetic (one copy) ----------------------------------------------------------
def filter_slot(n):
    """Neuron n = 32 j + b: its filter block g, low bit lb, high bit hb and
    id class jh = j >> 13 (any id width; the handle admits 24 bits)."""
    n = np.asarray(n).astype(np.uint64)
    b, j = n & 31, n >> 5
    jh = j >> 13
    t = jh * 0x9E5
    return (j ^ t) & (FILTER_BLOCKS - 1), b, (b + t) & 31, jh


def _src_code(n):
    """abnn.h (abnn_state): the filter code of a 24-bit src, as (lo, hi)."""
    g, b, hb, jh = filter_slot(np.asarray(n).astype(np.uint64) & 0xFFFFFF)
    return (g << 3 | (hb & 7)), (b | (jh >> 5) << 5 | (hb >> 3) << 6)


def _code_src(lo, hi):
    g, b = lo >> 3, hi & 31
    hb = (lo & 7) | (hi >> 6) << 3
    jh = (((hb - b) * 13) & 31) | ((hi >> 5) & 1) << 5
    j = ((g ^ jh * 0x9E5) & 8191) | jh << 13
    return j << 5 | b


def f2_hashes(n):
    """engine.h f2_hash1 / f2_hash2: two 16-bit positions in the 64 Ki-bit Bloom filter."""
    n = np.asarray(n).astype(np.uint64)
    m = np.uint64(0xFFFFFFFF)
    return ((n * np.uint64(0x9E3779B1)) & m) >> 16, ((n * np.uint64(0x85EBCA77) + np.uint64(0x165667B1)) & m) >> 16


# ---- numpy model of the two filters ---------------------------------------------------------------
def filter_model(recent_ids):
    """filter_set restated: the {low, high} images of the recent set, each as
    bool[8192, 32] (bit b of block g)."""
    g, lb, hb, _ = filter_slot(recent_ids)
    g = g.astype(np.int64)
    low, high = np.zeros((FILTER_BLOCKS, 32), bool), np.zeros((FILTER_BLOCKS, 32), bool)
    low[g, lb.astype(np.int64)] = True
    high[g, hb.astype(np.int64)] = True
    return low, high


def passes_filter(model, src):
    """The gate's filter test of every src: low bit lb and high bit hb of its block."""
    low, high = model
    g, lb, hb, _ = filter_slot(src)
    g = g.astype(np.int64)
    return low[g, lb.astype(np.int64)] & high[g, hb.astype(np.int64)]


def f2_model(recent_ids):
    bits = np.zeros(F2_WORDS * 32, bool)
    h1, h2 = f2_hashes(recent_ids)
    bits[h1.astype(np.int64)] = True
    bits[h2.astype(np.int64)] = True
    return bits


def passes_f2(bits, src):
    h1, h2 = f2_hashes(src)
    return bits[h1.astype(np.int64)] & bits[h2.astype(np.int64)]


def recent_mask(last_fired_at_start, now, window=WINDOW_PRE):
    """age32(now, lastFired) <= window per neuron (ages are u32)."""
    age = np.uint32(int(now) & 0xFFFFFFFF) - last_fired_at_start.astype(np.uint32)  # wraps
    return age <= np.uint32(window)


# ---- the debug bitmap -----------------------------------------------------------------------------
def _bitmap(g):
    import ctypes as C
    nw = 2 * ((g.n_neuron() + 63) // 64)
    out = np.zeros(nw, dtype=np.uint32)
    inc = C.c_int(0)
    f = g._lib.abnn_debug_bitmap
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_int)]
    f.restype = C.c_int
    assert f(g._h, out.ctypes.data, nw, C.byref(inc)) == 0
    return out, bool(inc.value)


def _expected_bitmap(last_fired_at_start, now, n_words, window=WINDOW_PRE):
    bits = recent_mask(last_fired_at_start, now, window).astype(np.uint8)
    bits = np.concatenate([bits, np.zeros(n_words * 32 - bits.size, np.uint8)])
    return np.packbits(bits.reshape(-1, 32)[:, ::-1], axis=1).view(">u4").ravel().astype(np.uint32)


# ---- the crafted graph ----------------------------------------------------------------------------
N_IN = N_OUT = 256
L1_PER_PROBE, L1_PER_ALIAS_PROBE, L2_PER_PROBE, PER_DECOY = 3, 8, 5, 4
N_TRIPLES, N_F2_DECOYS = 40, 24


def fixed_ids(n_nrn):
    """The ids every crafted graph probes whatever its seed: each class's first
    and last id, and the ids around the first fold (2^18), the x bit (2^23)
    and the end of the partial last bitmap word."""
    n_classes = (n_nrn - 1 >> CLASS_LOG2) + 1
    ids = []
    for c in range(n_classes):
        ids += [c << CLASS_LOG2, min(((c + 1) << CLASS_LOG2) - 1, n_nrn - 1)]
    ids += [v for v in ((1 << 18) - 1, 1 << 18, (1 << 23) - 1, 1 << 23, n_nrn - 1) if v < n_nrn]
    return np.unique(np.array(ids, dtype=np.int64))


def _id_of(jh, g, b):
    """The id of class jh whose word folds onto block g, bit b (filter_slot's inverse)."""
    jl = (g ^ (jh * 0x9E5)) & (FILTER_BLOCKS - 1)
    return ((jh << 13 | jl) << 5) | b


@functools.lru_cache(maxsize=4)
def high_id_parts(n_nrn, n_syn=1_000_000, seed=11):
    """The crafted graph and what it was crafted from: dict of `syn` (SYN_DTYPE,
    read-only), `probes`, `decoys` (every alias decoy), `f2_decoys` (the
    decoys that the probes also cover in the Bloom filter) and `triples`
    (rows A, B, D)."""
    from oracle import oracle as O

    rng = np.random.default_rng(seed)
    syn = O.gen_synapses(0, n_syn, N_IN, N_OUT, n_nrn, seed, nthreads=16)
    n_classes = (n_nrn - 1 >> CLASS_LOG2) + 1

    # probes: a dozen random ids per class, an id with b = 31 and one with b = 0, the fixed ids
    probes = [fixed_ids(n_nrn)]
    for c in range(n_classes):
        lo, hi = c << CLASS_LOG2, min((c + 1) << CLASS_LOG2, n_nrn)
        probes.append(rng.integers(lo, hi, 12))
        w = rng.integers(lo >> 5, (hi - 1 >> 5) + 1, 2) << 5
        probes.append(np.array([min(w[0] + 31, hi - 1), w[1]]))
    probes = np.unique(np.concatenate(probes))
    probes = probes[probes >= N_IN]  # (inputs are stamped by the stimulus anyway)

    # alias triples from the code arithmetic: D shares A's block and low bit and
    # B's block and high bit, the three in different classes (different t mod
    # 32, so that neither A nor B alone sets both of D's bits)
    taken = set(probes.tolist()) | set(syn["dst"].tolist())
    cand = np.zeros((0, 3), np.int64)  # (A, B, D)
    if n_classes >= 3:
        ga, ba, _, ca = (x.astype(np.int64)[:, None] for x in filter_slot(probes))
        cd = np.arange(n_classes, dtype=np.int64)[None, :]  # every class for D,
        cb = rng.integers(0, n_classes, (probes.size, n_classes))  # a random one for B
        d = _id_of(cd, ga, ba)
        b = _id_of(cb, ga, ((ba + cd * 0x9E5) - cb * 0x9E5) & 31)
        ok = (ca % 32 != cb % 32) & (ca % 32 != cd % 32) & (cb % 32 != cd % 32)
        ok &= (d >= 512) & (d < n_nrn) & (b >= 512) & (b < n_nrn)
        known = np.fromiter(taken, np.int64)
        ok &= ~np.isin(d, known) & ~np.isin(b, known)
        a = np.broadcast_to(probes[:, None], d.shape)
        cand = np.stack([a[ok], b[ok], d[ok]], axis=1)
        cand = cand[rng.permutation(len(cand))]
    # ... of which the ones whose two Bloom bits the probes cover come first:
    # once A, B and those probes are recent, only the exact bitmap rejects D
    covered = passes_f2(f2_model(probes), cand[:, 2]) if len(cand) else np.zeros(0, bool)
    pick_f2 = np.flatnonzero(covered)[:N_F2_DECOYS]
    rest = np.flatnonzero(~covered)[:8 * N_TRIPLES]
    triples, used = [], set()
    for i in list(pick_f2) + list(rest):
        a, b, d = cand[i]
        if b in used or d in used:
            continue
        if len(triples) >= len(pick_f2) + N_TRIPLES:
            break
        triples.append((a, b, d, bool(covered[i])))
        used |= {int(b), int(d)}
    tri = np.array([t[:3] for t in triples], dtype=np.int64).reshape(-1, 3)
    f2_decoys = np.array([t[2] for t in triples if t[3]], dtype=np.int64)
    decoys = tri[:, 2].copy()
    probes = np.unique(np.concatenate([probes, tri[:, 1]]))

    # the crafted records, at random positions of the array
    def targets(n):
        return rng.integers(N_IN, n_nrn, n)

    # (a triple's A and B get more input records: each fires 0.65 of the time,
    # and the triple's decoy aliases only while both are recent)
    l1_dst = np.concatenate([np.repeat(probes, L1_PER_PROBE),
                             np.repeat(tri[:, :2].ravel(), L1_PER_ALIAS_PROBE - L1_PER_PROBE)])
    l2_src = np.repeat(probes, L2_PER_PROBE)
    dc_src = np.repeat(decoys, PER_DECOY)
    src = np.concatenate([rng.integers(0, N_IN, l1_dst.size), l2_src, dc_src])
    dst = np.concatenate([l1_dst, targets(l2_src.size), targets(dc_src.size)])
    dst[np.isin(dst, decoys)] = N_IN  # a decoy is never stamped
    w = np.concatenate([np.full(l1_dst.size, 0.9), np.full(l2_src.size + dc_src.size, 0.3)]).astype(np.float32)
    assert src.size <= n_syn // 4
    at = rng.choice(n_syn, src.size, replace=False)
    syn["src"][at], syn["dst"][at], syn["w"][at] = src, dst, w
    assert not np.isin(syn["dst"], decoys).any()
    syn.setflags(write=False)
    return dict(syn=syn, probes=probes, decoys=decoys, f2_decoys=f2_decoys, triples=tri, crafted_at=np.sort(at))


def high_id_graph(n_nrn, n_syn=1_000_000, seed=11):
    """SYN_DTYPE records (a fresh copy): oracle.gen_synapses at n_nrn neurons
    with the crafted records of high_id_parts written over random positions."""
    return high_id_parts(n_nrn, n_syn, seed)["syn"].copy()
