"""The graph builder (abnn.h ``abnn_graph_*`` / ``abnn_build_graph``, DESIGN.md
§9) on the host side.

The builder itself runs in the HIP library (csrc/graph.hip, the rule in
csrc/graph.h); this module holds what needs no GPU: the block and weight-law
constructors, the spec, the validator (:func:`records`) and the numpy
restatement of the rule (:func:`reference`: the test reference, and usable for
small graphs).  A graph is up to 16 blocks laid end to end; every record is a
closed-form function of (seed, block number, index in the block), built from
64-bit integer draws, 24-bit uniforms and three fp32 operations, so
:func:`reference` equals the device and ``abnn_graph_fill_host`` bit for bit.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

from ._lib import (GRAPH_KEY, GRAPH_MAX_BLOCKS, TOPO_DENSE, TOPO_RANDOM, TOPO_RING, W_BETA, W_UNIFORM, GraphBlock,
                   GraphSpec)

F32 = np.float32
U32 = np.uint32
U64 = np.uint64
# the interchange record (brain.SYN_DTYPE)
SYN_DTYPE = np.dtype([("src", "<u4"), ("dst", "<u4"), ("w", "<f4"), ("pad", "<f4")])
MAX_DRAWS = 15  # Beta: a + b - 1
_CHUNK = 1 << 20  # records per numpy step of reference()

WeightLaw = Tuple[int, float, float, int, int]  # (law, w_lo, w_hi, beta_a, beta_b)
Population = Sequence[int]  # (first, count)


# ---- weight laws ------------------------------------------------------------------------------
def uniform(lo: float, hi: float) -> WeightLaw:
    """w ~ U[lo, hi): lo + u * (hi - lo), u a 24-bit uniform."""
    return (W_UNIFORM, float(lo), float(hi), 0, 0)


def beta(a: int, b: int, lo: float = 0.0, hi: float = 1.0) -> WeightLaw:
    """w = lo + v * (hi - lo), v ~ Beta(a, b) for integers a, b >= 1 with
    a + b - 1 <= 15: the a-th smallest of a + b - 1 uniforms (README §6 asks for
    Beta(2, 8): the second smallest of nine)."""
    return (W_BETA, float(lo), float(hi), int(a), int(b))


# ---- blocks -----------------------------------------------------------------------------------
def _block(count, src, dst, topology, k, p, weights: WeightLaw) -> GraphBlock:
    law, lo, hi, a, b = weights
    return GraphBlock(int(count), int(src[0]), int(src[1]), int(dst[0]), int(dst[1]), int(topology), int(k), float(p),
                      int(law), lo, hi, a, b)


def dense(src: Population, dst: Population, weights: WeightLaw, count: Optional[int] = None) -> GraphBlock:
    """All-to-all, row-major: record r is src[r // D % S] -> dst[r % D];
    ``count`` defaults to S * D (one copy of every pair)."""
    return _block(int(src[1]) * int(dst[1]) if count is None else count, src, dst, TOPO_DENSE, 0, 0.0, weights)


def random(src: Population, dst: Population, count: int, weights: WeightLaw) -> GraphBlock:
    """``count`` edges with src and dst uniform and independent over their
    populations (Erdős–Rényi G(n, M) with replacement: multi-edges and
    self-loops allowed, as brain-engine.cpp:46-47)."""
    return _block(count, src, dst, TOPO_RANDOM, 0, 0.0, weights)


def small_world(pop: Population, k: int, p: float, weights: WeightLaw, count: Optional[int] = None) -> GraphBlock:
    """Directed Watts–Strogatz over one population of n nodes: the ring lattice
    i -> i+1, i-1, i+2, i-2, ... of out-degree ``k`` (1 <= k < n), each edge
    rewired with probability ``p`` to a uniform other node (never a self-loop).
    ``count`` defaults to n * k."""
    return _block(int(pop[1]) * int(k) if count is None else count, pop, pop, TOPO_RING, k, p, weights)


def spec(blocks: Sequence[GraphBlock], seed: int = 1) -> GraphSpec:
    """The blocks laid end to end in global record order under one seed.  The
    spec is not validated here: :func:`records` (or the library) does that."""
    blocks = list(blocks)
    if len(blocks) > GRAPH_MAX_BLOCKS:
        raise ValueError(f"graph: at most {GRAPH_MAX_BLOCKS} blocks")
    s = GraphSpec(int(seed) & (2**64 - 1), len(blocks), 0)
    for j, b in enumerate(blocks):
        s.blocks[j] = GraphBlock.from_buffer_copy(bytes(b))  # a copy: the spec owns its blocks
    return s


def recipe(n_input: int, n_output: int, n_hidden: int, n_syn: int, seed: int = 1) -> GraphSpec:
    """A two-block spec with the SHAPE of build_random_graph
    (brain-engine.cpp:31-53, ``Brain.build_random_graph``): the dense
    input -> output block with w ~ U(0.4, 0.8), then n_syn - n_input * n_output
    random hidden -> hidden edges with w ~ U(0.1, 0.2).  The same shape, not
    the same bits: the builder's draw streams (keyed per block) differ from
    abnn_generate_synapses', so the records differ while their statistics
    agree.  With n_syn <= n_input * n_output only (a prefix of) the dense block."""
    n_io = int(n_input) * int(n_output)
    blocks = []
    if n_io:
        blocks.append(dense((0, n_input), (n_input, n_output), uniform(0.4, 0.8), count=min(n_io, int(n_syn))))
    if int(n_syn) > n_io:
        hid = (int(n_input) + int(n_output), int(n_hidden))
        blocks.append(random(hid, hid, int(n_syn) - n_io, uniform(0.1, 0.2)))
    return spec(blocks, seed)


# ---- the validator ----------------------------------------------------------------------------
def _bits(x: float) -> int:
    return int(np.array([x], dtype=F32).view(U32)[0])


def _block_ok(b: GraphBlock) -> bool:
    if not 1 <= b.count < 1 << 59:
        return False
    if b.src_count == 0 or b.dst_count == 0:
        return False
    if b.src_first + b.src_count > 1 << 32 or b.dst_first + b.dst_count > 1 << 32:
        return False
    if b.reserved[0] or b.reserved[1]:
        return False
    if b.topology == TOPO_RING:
        if b.src_first != b.dst_first or b.src_count != b.dst_count:
            return False
        if not 1 <= b.k < b.src_count:
            return False
        if not F32(0.0) <= F32(b.p_rewire) <= F32(1.0):  # false for NaN
            return False
    elif b.topology in (TOPO_DENSE, TOPO_RANDOM):
        if b.k or _bits(b.p_rewire):
            return False
    else:
        return False
    if b.weight_law == W_BETA:
        if b.beta_a == 0 or b.beta_b == 0 or b.beta_a + b.beta_b - 1 > MAX_DRAWS:
            return False
    elif b.weight_law == W_UNIFORM:
        if b.beta_a or b.beta_b:
            return False
    else:
        return False
    if not (np.isfinite(F32(b.w_lo)) and np.isfinite(F32(b.w_hi))):
        return False
    return bool(F32(b.w_lo) <= F32(b.w_hi))


def records(s: Optional[GraphSpec]) -> int:
    """abnn_graph_records: the sum of the counts, or 0 for an invalid spec."""
    if s is None or not 1 <= s.n_blocks <= GRAPH_MAX_BLOCKS or s.reserved:
        return 0
    if not all(_block_ok(s.blocks[j]) for j in range(s.n_blocks)):
        return 0
    if any(bytes(s.blocks[j]).strip(b"\0") for j in range(s.n_blocks, GRAPH_MAX_BLOCKS)):
        return 0
    return sum(int(s.blocks[j].count) for j in range(s.n_blocks))


# ---- the rule in numpy ------------------------------------------------------------------------
_M64 = (1 << 64) - 1


def _splitmix64_at(seed: int, k: np.ndarray) -> np.ndarray:
    """splitmix64_at over an array of counters, u64 wrap-around."""
    with np.errstate(over="ignore"):
        z = U64(seed) + (k + U64(1)) * U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def _draw(key: int, r: np.ndarray, c: int) -> np.ndarray:
    return _splitmix64_at(key, (r << U64(5)) | U64(c))


def _unit24(x: np.ndarray) -> np.ndarray:
    return (x >> U64(40)).astype(F32) * F32(1.0 / 16777216.0)


def _pick(x: np.ndarray, n: int) -> np.ndarray:
    return (((x >> U64(32)) * U64(n)) >> U64(32)).astype(np.int64)


def _block_records(b: GraphBlock, key: int, r: np.ndarray) -> np.ndarray:
    """Records ``r`` (np.uint64 indices within the block) of block ``b``."""
    out = np.zeros(len(r), dtype=SYN_DTYPE)
    S, D = int(b.src_count), int(b.dst_count)
    if b.topology == TOPO_DENSE:
        src = (r // U64(D)) % U64(S) + U64(b.src_first)
        dst = r % U64(D) + U64(b.dst_first)
    elif b.topology == TOPO_RANDOM:
        src = _pick(_draw(key, r, 0), S) + b.src_first
        dst = _pick(_draw(key, r, 1), D) + b.dst_first
    else:
        n, k = S, int(b.k)
        i = ((r // U64(k)) % U64(n)).astype(np.int64)
        q = (r % U64(k)).astype(np.int64)
        o = (q >> 1) + 1
        t = (i + np.where(q & 1, n - o, o)) % n
        rewired = _unit24(_draw(key, r, 0)) < F32(b.p_rewire)
        t = np.where(rewired, (i + 1 + _pick(_draw(key, r, 1), n - 1)) % n, t)
        src, dst = i + b.src_first, t + b.src_first
    out["src"] = src.astype(U32)
    out["dst"] = dst.astype(U32)
    if b.weight_law == W_BETA:
        m = int(b.beta_a) + int(b.beta_b) - 1
        draws = np.stack([_unit24(_draw(key, r, 2 + c)) for c in range(m)], axis=1) if len(r) else \
            np.zeros((0, m), dtype=F32)
        v = np.sort(draws, axis=1)[:, int(b.beta_a) - 1]
    else:
        v = _unit24(_draw(key, r, 2))
    span = F32(b.w_hi) - F32(b.w_lo)  # three separate fp32 operations
    scaled = (v.astype(F32) * span).astype(F32)
    out["w"] = (F32(b.w_lo) + scaled).astype(F32)
    return out


def reference(s: GraphSpec, first: int = 0, n: Optional[int] = None) -> np.ndarray:
    """Global records [first, first + n) of the spec (default: to the end) by
    the rule of abnn.h in vectorised numpy, as SYN_DTYPE."""
    total = records(s)
    if total == 0:
        raise ValueError("graph: invalid spec")
    first = int(first)
    n = total - first if n is None else int(n)
    if first < 0 or n < 0 or first + n > total:
        raise ValueError("graph: the range ends past records(spec)")
    out = np.zeros(n, dtype=SYN_DTYPE)
    start = 0
    for j in range(s.n_blocks):
        b = s.blocks[j]
        lo, hi = max(first, start), min(first + n, start + int(b.count))
        key = (int(s.seed) ^ (GRAPH_KEY * (j + 1))) & _M64
        for at in range(lo, hi, _CHUNK):
            stop = min(hi, at + _CHUNK)
            r = np.arange(at - start, stop - start, dtype=U64)
            out[at - first:stop - first] = _block_records(b, key, r)
        start += int(b.count)
    return out
