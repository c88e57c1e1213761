// graph.h -- the device-side graph builder (graph.hip; abnn.h abnn_graph_* /
// abnn_build_graph): a graph as up to 16 blocks laid end to end,
// every record a closed-form function of (seed, block, index in the block).
// The rule lives here ONCE, as __host__ __device__ inlines: the kernel
// (graph.hip k_build_graph) and abnn_graph_fill_host (capi.hip) both call
// graph_start / graph_emit / graph_step, so they cannot drift apart.
#pragma once

#include "engine.h"

namespace abnn {

constexpr int kGraphThreads = 256;      // 4 waves per workgroup
constexpr uint32_t kGraphQuad = 4;      // consecutive local records per lane and iteration
constexpr uint32_t kGraphKeep = 8;      // Beta: order statistics kept in registers (min(a, b) <= 8)
constexpr uint32_t kGraphMaxDraws = 15; // Beta: a + b - 1

// The checks of abnn_graph_records for one block (everything that needs no handle).
inline bool graph_block_ok(const abnn_graph_block& b)
{
    if (b.count == 0 || b.count >= (1ull << 59)) return false;
    if (b.src_count == 0 || b.dst_count == 0) return false;
    if ((uint64_t)b.src_first + b.src_count > (1ull << 32)) return false;
    if ((uint64_t)b.dst_first + b.dst_count > (1ull << 32)) return false;
    if (b.reserved[0] != 0 || b.reserved[1] != 0) return false;
    uint32_t p_bits;
    __builtin_memcpy(&p_bits, &b.p_rewire, 4);
    if (b.topology == ABNN_TOPO_RING) {
        if (b.src_first != b.dst_first || b.src_count != b.dst_count) return false;
        if (b.k == 0 || b.k >= b.src_count) return false;
        if (!(b.p_rewire >= 0.0f && b.p_rewire <= 1.0f)) return false;  // false for NaN too
    } else if (b.topology == ABNN_TOPO_DENSE || b.topology == ABNN_TOPO_RANDOM) {
        if (b.k != 0 || p_bits != 0) return false;  // +0.0f
    } else {
        return false;
    }
    if (b.weight_law == ABNN_W_BETA) {
        if (b.beta_a == 0 || b.beta_b == 0) return false;
        if ((uint64_t)b.beta_a + b.beta_b - 1 > kGraphMaxDraws) return false;
    } else if (b.weight_law == ABNN_W_UNIFORM) {
        if (b.beta_a != 0 || b.beta_b != 0) return false;
    } else {
        return false;
    }
    const float inf = __builtin_inff();
    if (!(b.w_lo > -inf && b.w_lo < inf && b.w_hi > -inf && b.w_hi < inf)) return false;  // finite, not NaN
    if (!(b.w_lo <= b.w_hi)) return false;
    return true;
}

// abnn_graph_records: the sum of the counts, or 0 for an invalid spec.
inline uint64_t graph_records(const abnn_graph_spec* s)
{
    if (!s || s->n_blocks < 1 || s->n_blocks > ABNN_GRAPH_MAX_BLOCKS || s->reserved != 0) return 0;
    uint64_t total = 0;  // <= 16 * 2^59: no wrap
    for (uint32_t j = 0; j < s->n_blocks; ++j) {
        if (!graph_block_ok(s->blocks[j])) return 0;
        total += s->blocks[j].count;
    }
    const unsigned char* tail = reinterpret_cast<const unsigned char*>(s->blocks + s->n_blocks);
    const unsigned char* end = reinterpret_cast<const unsigned char*>(s->blocks + ABNN_GRAPH_MAX_BLOCKS);
    for (; tail != end; ++tail)
        if (*tail) return 0;
    return total;
}

// The spec as the kernel takes it (by value): the blocks and their first
// global records, start[n_blocks] = the total, the entries past it ~0.
struct GraphTable {
    uint64_t seed;
    uint32_t n_blocks, pad;
    uint64_t start[ABNN_GRAPH_MAX_BLOCKS + 1];
    abnn_graph_block blocks[ABNN_GRAPH_MAX_BLOCKS];
};

inline GraphTable graph_table(const abnn_graph_spec& s)  // of a valid spec
{
    GraphTable t;
    __builtin_memset(&t, 0, sizeof(t));
    t.seed = s.seed;
    t.n_blocks = s.n_blocks;
    uint64_t at = 0;
    for (uint32_t j = 0; j <= ABNN_GRAPH_MAX_BLOCKS; ++j) {
        t.start[j] = j <= s.n_blocks ? at : ~0ull;
        if (j < s.n_blocks) {
            t.blocks[j] = s.blocks[j];
            at += s.blocks[j].count;
        }
    }
    return t;
}

// The block of global record g < the total: the last j with start[j] <= g.
__host__ __device__ inline uint32_t graph_block_of(const GraphTable& t, uint64_t g)
{
    uint32_t j = 0;
#pragma unroll
    for (uint32_t i = 1; i < ABNN_GRAPH_MAX_BLOCKS; ++i) j += (i < t.n_blocks && t.start[i] <= g) ? 1u : 0u;
    return j;
}

// splitmix64_at of kernels.hip (the library's counter-based generator), for both sides
__host__ __device__ inline uint64_t graph_splitmix64_at(uint64_t seed, uint64_t k)
{
    uint64_t z = seed + (k + 1u) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__host__ __device__ inline uint64_t graph_key(uint64_t seed, uint32_t j) { return seed ^ (ABNN_GRAPH_KEY * (uint64_t)(j + 1u)); }

// X(c) of record r
__host__ __device__ inline uint64_t graph_draw(uint64_t key, uint64_t r, uint32_t c)
{
    return graph_splitmix64_at(key, (r << 5) | c);
}

// pick(c, n): the multiply-shift of the existing recipe
__host__ __device__ inline uint32_t graph_pick(uint64_t x, uint32_t n) { return (uint32_t)(((x >> 32) * n) >> 32); }

// Where record r of a block stands in its topology: (a, b) = ((r / D) % S,
// r % D) for DENSE, (i, q) = ((r / k) % n, r % k) for RING, unused for RANDOM.
// graph_start divides; graph_step moves to record r + 1 without dividing.
struct GraphPos {
    uint32_t a, b;
};

// (kTopo: the block's topology when known at compile time, as graph_emit's.)
template <int kTopo = -1>
__host__ __device__ inline GraphPos graph_start(const abnn_graph_block& blk, uint64_t r)
{
    const uint32_t topo = kTopo < 0 ? blk.topology : (uint32_t)kTopo;
    GraphPos p = {0u, 0u};
    if (topo == ABNN_TOPO_RANDOM) return p;
    const uint32_t inner = topo == ABNN_TOPO_RING ? blk.k : blk.dst_count;
    const uint32_t outer = blk.src_count;
    if ((r >> 32) == 0) {  // the same quotients, in 32 bits
        const uint32_t r32 = (uint32_t)r, quot = r32 / inner;
        p.b = r32 - quot * inner;
        p.a = quot % outer;
    } else {
        const uint64_t quot = r / inner;
        p.b = (uint32_t)(r - quot * inner);
        p.a = (uint32_t)(quot % outer);
    }
    return p;
}

template <int kTopo = -1>
__host__ __device__ inline void graph_step(const abnn_graph_block& blk, GraphPos& p)
{
    const uint32_t topo = kTopo < 0 ? blk.topology : (uint32_t)kTopo;
    if (topo == ABNN_TOPO_RANDOM) return;  // never reads p
    const uint32_t inner = topo == ABNN_TOPO_RING ? blk.k : blk.dst_count;
    if (++p.b == inner) {
        p.b = 0;
        if (++p.a == blk.src_count) p.a = 0;
    }
}

// The Beta(a, b) order statistic as 24-bit integers (unit24 is monotone and
// exact on them): the a-th smallest of m = a + b - 1 draws is the b-th
// largest, so min(a, b) <= 8 values are kept, by an insertion network, never
// a sort of all fifteen.
__host__ __device__ inline uint32_t graph_beta24(uint64_t key, uint64_t r, uint32_t a, uint32_t b)
{
    const uint32_t m = a + b - 1u;
    const bool low = a <= b;            // keep the a smallest; else the b largest, as the smallest complements
    const uint32_t keep = low ? a : b;  // 1 .. 8
    const uint32_t flip = low ? 0u : 0xFFFFFFu;
    uint32_t s[kGraphKeep];
#pragma unroll
    for (uint32_t i = 0; i < kGraphKeep; ++i) s[i] = 0xFFFFFFFFu;
    for (uint32_t c = 0; c < m; ++c) {
        uint32_t x = (uint32_t)(graph_draw(key, r, 2u + c) >> 40) ^ flip;  // 24 bits; ^ flip = 0xFFFFFF - x
#pragma unroll
        for (uint32_t i = 0; i < kGraphKeep; ++i) {  // s stays sorted ascending: the 8 smallest so far
            const uint32_t lo = x < s[i] ? x : s[i];
            x = x < s[i] ? s[i] : x;
            s[i] = lo;
        }
    }
    uint32_t v = s[0];
#pragma unroll
    for (uint32_t i = 1; i < kGraphKeep; ++i) v = (i + 1u == keep) ? s[i] : v;
    return v ^ flip;
}

// Record r of block blk (number j through key = graph_key(seed, j)) at position
// p.  kTopo / kLaw: the block's topology and weight law when the caller knows
// them at compile time (the kernel's uniform path: straight-line code, the four
// records of a quad interleave), or -1 to read them from the block.
template <int kTopo = -1, int kLaw = -1>
__host__ __device__ inline void graph_emit(const abnn_graph_block& blk, uint64_t key, uint64_t r, const GraphPos& p,
                                           uint32_t& src, uint32_t& dst, float& w)
{
    const uint32_t topo = kTopo < 0 ? blk.topology : (uint32_t)kTopo;
    const uint32_t law = kLaw < 0 ? blk.weight_law : (uint32_t)kLaw;
    if (topo == ABNN_TOPO_DENSE) {
        src = blk.src_first + p.a;
        dst = blk.dst_first + p.b;
    } else if (topo == ABNN_TOPO_RANDOM) {
        src = blk.src_first + graph_pick(graph_draw(key, r, 0u), blk.src_count);
        dst = blk.dst_first + graph_pick(graph_draw(key, r, 1u), blk.dst_count);
    } else {  // RING: sums below 2 n <= 2^33, one conditional subtraction is the % n
        const uint64_t n = blk.src_count, i = p.a;
        const uint32_t q = p.b, o = (q >> 1) + 1u;
        uint64_t t = i + ((q & 1u) ? n - o : (uint64_t)o);
        const float u0 = (float)(graph_draw(key, r, 0u) >> 40) * (1.0f / 16777216.0f);
        if (u0 < blk.p_rewire) t = i + 1u + graph_pick(graph_draw(key, r, 1u), (uint32_t)(n - 1u));
        if (t >= n) t -= n;
        src = blk.src_first + (uint32_t)i;
        dst = blk.src_first + (uint32_t)t;
    }
    const uint32_t v24 = law == ABNN_W_BETA ? graph_beta24(key, r, blk.beta_a, blk.beta_b)
                                            : (uint32_t)(graph_draw(key, r, 2u) >> 40);
    const float v = (float)v24 * (1.0f / 16777216.0f);  // unit24
    const float span = blk.w_hi - blk.w_lo;               // three separate fp32 operations (-ffp-contract=off)
    const float scaled = v * span;
    w = blk.w_lo + scaled;
}

// Global records [first, first + n) of a valid spec into out (the host side of the rule).
inline void graph_fill(const GraphTable& t, uint64_t first, uint64_t n, abnn_synapse* out)
{
    uint64_t g = first;
    const uint64_t end = first + n;
    while (g < end) {
        const uint32_t j = graph_block_of(t, g);
        const abnn_graph_block& blk = t.blocks[j];
        const uint64_t key = graph_key(t.seed, j);
        const uint64_t stop = t.start[j + 1] < end ? t.start[j + 1] : end;
        uint64_t r = g - t.start[j];
        GraphPos p = graph_start(blk, r);
        for (; g < stop; ++g, ++r, graph_step(blk, p)) {
            abnn_synapse& o = out[g - first];
            graph_emit(blk, key, r, p, o.src, o.dst, o.w);
            o.pad = 0.0f;
        }
    }
}

// Fills local records [0, n_syn) of `a` with global records syn_offset + k of
// the table (a valid spec whose total covers them), asynchronously on `s`:
// a persistent grid-stride launch of at most `blocks` workgroups.  Nothing at
// or past n_syn is written.  nt: non-temporal stores.
hipError_t launch_build_graph(const SynArrays& a, uint64_t n_syn, uint64_t syn_offset, const GraphTable& t,
                              uint32_t blocks, bool nt, hipStream_t s);

}  // namespace abnn
