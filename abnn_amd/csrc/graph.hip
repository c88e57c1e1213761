// graph.hip -- the device-side graph builder (abnn.h abnn_build_graph,
// DESIGN.md §9): local records [0, n_syn) of a handle from a block spec, every
// record the closed-form function of graph.h (graph_start / graph_emit /
// graph_step: the same inlines abnn_graph_fill_host runs on the host).
//
//   k_build_graph<kNT> : a persistent grid-stride launch.  Per iteration a
//       lane takes one QUAD: four consecutive local records, aligned to 4, so
//       that its stores are whole dwords -- 8 B of lo, 4 B of hi, two 16-B
//       stores of {dst, w} and, in random mode, 16 B of the src32 mirror (the
//       2-byte and 1-byte stores of set_src cost 4 store instructions per
//       record; these are 4 or 5 per quad).
//       A wave's 64 quads are 256 consecutive records.  When all of them lie
//       in one block and below n_syn -- every wave but the at most 16 that
//       straddle a block boundary and the last one -- the block is found once
//       per wave with scalar compares and its parameters are scalar loads, so
//       the topology and weight-law branches are uniform: no divergence.  The
//       lane divides once (graph_start: r / D, r / k, % n; in 32 bits while
//       r < 2^32) and steps through its four records.
//       The other waves take the boundary path: a scalar loop over the blocks
//       that the wave touches, every record starting from its own division; a
//       quad that reaches n_syn stores its records one by one, so nothing at or
//       past n_syn is written (the padding stays zero, engine.h kDummyRecords).
//       The local quad is aligned, the global record syn_offset + k need not
//       be: a shard whose offset is odd or a block boundary inside a quad only
//       takes the boundary path.
#include "graph.h"
#include "scan.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace abnn {
namespace {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <bool kNT, typename T>
__device__ __forceinline__ void put(T* p, T v)
{
    if constexpr (kNT)
        __builtin_nontemporal_store(v, p);
    else
        *p = v;
}

// The four records of the full quad at local record k0 (k0 % 4 == 0, k0 + 4 <= n_syn).
template <bool kNT>
__device__ __forceinline__ void store_quad(const SynArrays& a, uint64_t k0, const uint32_t (&src)[4],
                                           const uint32_t (&dst)[4], const float (&w)[4])
{
    uint32_t c[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) c[e] = src_code(src[e]);
    u32x2 lo;
    lo.x = (c[0] & 0xFFFFu) | c[1] << 16;
    lo.y = (c[2] & 0xFFFFu) | c[3] << 16;
    const uint32_t hi = (c[0] >> 16 & 0xFFu) | (c[1] >> 16 & 0xFFu) << 8 | (c[2] >> 16 & 0xFFu) << 16 | (c[3] >> 16) << 24;
    put<kNT>(reinterpret_cast<u32x2*>(a.lo + k0), lo);
    put<kNT>(reinterpret_cast<uint32_t*>(a.hi + hi_pos(k0)), hi);
    u32x4 d0, d1;
    d0.x = dst[0], d0.y = __float_as_uint(w[0]), d0.z = dst[1], d0.w = __float_as_uint(w[1]);
    d1.x = dst[2], d1.y = __float_as_uint(w[2]), d1.z = dst[3], d1.w = __float_as_uint(w[3]);
    put<kNT>(reinterpret_cast<u32x4*>(a.dw + k0), d0);
    put<kNT>(reinterpret_cast<u32x4*>(a.dw + k0 + 2), d1);
    if (a.src32) {
        u32x4 s;
        s.x = src[0], s.y = src[1], s.z = src[2], s.w = src[3];
        put<kNT>(reinterpret_cast<u32x4*>(a.src32 + k0), s);
    }
}

// One record on its own (the quad that reaches n_syn): set_src of kernels.hip.
__device__ __forceinline__ void store_one(const SynArrays& a, uint64_t k, uint32_t src, uint32_t dst, float w)
{
    const uint32_t c = src_code(src);
    a.lo[k] = (uint16_t)c;
    a.hi[hi_pos(k)] = (uint8_t)(c >> 16);
    if (a.src32) a.src32[k] = src;
    a.dw[k] = make_uint2(dst, __float_as_uint(w));
}

// The four records r .. r + 3 of one block: one division (graph_start), then steps.
template <int kTopo, int kLaw>
__device__ __forceinline__ void quad(const abnn_graph_block& blk, uint64_t key, uint64_t r, uint32_t (&src)[4],
                                     uint32_t (&dst)[4], float (&w)[4])
{
    GraphPos p = graph_start<kTopo>(blk, r);
#pragma unroll
    for (uint32_t e = 0; e < kGraphQuad; ++e) {
        graph_emit<kTopo, kLaw>(blk, key, r + e, p, src[e], dst[e], w[e]);
        graph_step<kTopo>(blk, p);
    }
}

template <bool kNT>
__global__ __launch_bounds__(kGraphThreads) void k_build_graph(SynArrays a, uint64_t n_syn, uint64_t syn_offset,
                                                               GraphTable t)
{
    constexpr uint64_t kWaveRecords = 64u * kGraphQuad;
    const uint64_t quads = (n_syn + kGraphQuad - 1) / kGraphQuad;
    const uint64_t stride = (uint64_t)gridDim.x * kGraphThreads;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    // wq: the wave's first quad (uniform), so the loop's trip count is per wave
    // the block the wave worked in last, held in scalar registers: its table
    // entry is looked up again only when the wave leaves [cur_first, cur_stop)
    uint32_t cur_j = 0;
    uint64_t cur_first = 0, cur_stop = 0, cur_key = 0;
    abnn_graph_block cur = t.blocks[0];
    for (uint64_t wq = (uint64_t)blockIdx.x * kGraphThreads + wave * 64u; wq < quads; wq += stride) {
        const uint64_t wk = wq * kGraphQuad, wg = syn_offset + wk;  // the wave's first local / global record
        const uint64_t k0 = wk + lane * kGraphQuad, g0 = wg + lane * kGraphQuad;
        if (wg < cur_first || wg >= cur_stop) {                     // scalar
            cur_j = graph_block_of(t, wg);
            cur_first = t.start[cur_j];
            cur_stop = t.start[cur_j + 1];
            cur_key = graph_key(t.seed, cur_j);
            cur = t.blocks[cur_j];
        }
        uint32_t j = cur_j;
        uint32_t src[4] = {0u, 0u, 0u, 0u}, dst[4] = {0u, 0u, 0u, 0u};
        float w[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (wg + kWaveRecords <= cur_stop && wk + kWaveRecords <= n_syn) {
            // every record of the wave in block j and below n_syn: one uniform
            // switch to the straight-line code of its topology and weight law
            const abnn_graph_block& blk = cur;
            const uint64_t key = cur_key, r = g0 - cur_first;
            switch (blk.topology * 2u + blk.weight_law) {
                case ABNN_TOPO_DENSE * 2u + ABNN_W_UNIFORM: quad<ABNN_TOPO_DENSE, ABNN_W_UNIFORM>(blk, key, r, src, dst, w); break;
                case ABNN_TOPO_DENSE * 2u + ABNN_W_BETA: quad<ABNN_TOPO_DENSE, ABNN_W_BETA>(blk, key, r, src, dst, w); break;
                case ABNN_TOPO_RANDOM * 2u + ABNN_W_UNIFORM: quad<ABNN_TOPO_RANDOM, ABNN_W_UNIFORM>(blk, key, r, src, dst, w); break;
                case ABNN_TOPO_RANDOM * 2u + ABNN_W_BETA: quad<ABNN_TOPO_RANDOM, ABNN_W_BETA>(blk, key, r, src, dst, w); break;
                case ABNN_TOPO_RING * 2u + ABNN_W_UNIFORM: quad<ABNN_TOPO_RING, ABNN_W_UNIFORM>(blk, key, r, src, dst, w); break;
                default: quad<ABNN_TOPO_RING, ABNN_W_BETA>(blk, key, r, src, dst, w); break;
            }
            store_quad<kNT>(a, k0, src, dst, w);
        } else {
            const uint64_t wave_end = wg + kWaveRecords;
            for (; j < t.n_blocks && t.start[j] < wave_end; ++j) {  // scalar: the blocks the wave touches
                const abnn_graph_block& blk = t.blocks[j];
                const uint64_t key = graph_key(t.seed, j), first = t.start[j], stop = t.start[j + 1];
#pragma unroll
                for (uint32_t e = 0; e < kGraphQuad; ++e) {
                    const uint64_t g = g0 + e;
                    if (k0 + e < n_syn && g >= first && g < stop) {
                        const uint64_t r = g - first;
                        const GraphPos p = graph_start(blk, r);
                        graph_emit(blk, key, r, p, src[e], dst[e], w[e]);
                    }
                }
            }
            if (k0 + kGraphQuad <= n_syn) {
                store_quad<kNT>(a, k0, src, dst, w);
            } else {
#pragma unroll
                for (uint32_t e = 0; e < kGraphQuad; ++e)
                    if (k0 + e < n_syn) store_one(a, k0 + e, src[e], dst[e], w[e]);
            }
        }
    }
}

}  // namespace

hipError_t launch_build_graph(const SynArrays& a, uint64_t n_syn, uint64_t syn_offset, const GraphTable& t,
                              uint32_t blocks, bool nt, hipStream_t s)
{
    if (n_syn == 0) return hipSuccess;
    const uint64_t quads = (n_syn + kGraphQuad - 1) / kGraphQuad;
    const uint64_t want = (quads + kGraphThreads - 1) / kGraphThreads;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(want, std::max(1u, blocks));
    if (nt)
        hipLaunchKernelGGL(k_build_graph<true>, dim3(grid), dim3(kGraphThreads), 0, s, a, n_syn, syn_offset, t);
    else
        hipLaunchKernelGGL(k_build_graph<false>, dim3(grid), dim3(kGraphThreads), 0, s, a, n_syn, syn_offset, t);
    return hipGetLastError();
}

}  // namespace abnn
