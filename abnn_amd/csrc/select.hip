// select.hip -- the synapse select (abnn.h abnn_select_*): the
// records of [0, n_syn) that match a src / dst / weight rule, compacted in
// record order, with their indices, into a caller-sized buffer.  Three launches
// in stream order; no workgroup waits for another (no look-back, no ticket, no
// residency assumption), so a select may run beside other streams' kernels.
//
//   k_select_count<kSrc> : a persistent grid-stride stream over tiles of
//       kSelectTile consecutive records; the stream is scan.h's (kSelectUnroll
//       loads in flight; kSrc: a src range is set).  A wave
//       adds its matches of a tile to the tile's u32 count (zeroed before the
//       launch; a wave without a match adds nothing), the workgroup its
//       tombstones to header word 1 with one atomic.
//   k_select_scan : the exclusive u64 prefix of the tile counts (the output
//       offset of every tile) and header words 0 and 2..4; one workgroup per
//       16 384 tiles, each summing the counts before its segment itself.
//   k_select_emit<kSrc> : a tile without a match, or whose offset is at or past
//       the capacity, is skipped without touching the records: a workgroup
//       looks at kSelectEmitChunk counts at once (tiles one grid apart) and
//       lists the tiles to emit.
//       Such a tile is re-read as the count launch read it; a match's rank in
//       the tile is the ballot / mbcnt rank inside its wave's load plus an LDS
//       prefix over the tile's (load, wave) totals.  A match below the capacity
//       stores its u64 index and its record {src, dst, w, 0} (one 16-B store);
//       without a src range its src is gathered from lo / hi here.
//
// A lane's record order: load k of the tile, lane, then the two records of the
// 16-B pair -- the index order.  Every count is an integer, every position
// offset + rank, so the result does not depend on the grid or on timing.
#include "select.h"
#include "scan.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace abnn {
namespace {

// the record plane starts 8 * (8 + capacity) bytes into the result: 8-byte aligned
typedef uint32_t u32x4a8 __attribute__((ext_vector_type(4), aligned(8)));
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

struct SelectArgs {
    RecordStream s;
    uint32_t* counts;             // [select_count_words(n)] matches per tile
    unsigned long long* offsets;  // [tiles] matches before the tile
    unsigned long long* out;
    uint64_t n, tiles, capacity, syn_offset;
    // ranges as {first, span}: x is inside iff x - first < span.  A range that
    // is not set has span 0xFFFFFFFF (every live value passes) without ANY and
    // span 0 (none does) with it
    uint32_t src_first, src_span, dst_first, dst_span;
    uint32_t any, weight;
    float w_lo, w_hi;
};

template <bool kSrc>
__device__ __forceinline__ bool match(const SelectArgs& a, uint32_t src, uint32_t dst, uint32_t wbits)
{
    if (dst == kAbsentDst) return false;  // a tombstone, or no record
    const bool D = dst - a.dst_first < a.dst_span;
    const bool S = kSrc ? src - a.src_first < a.src_span : a.any == 0;
    bool m = a.any ? (S || D) : (S && D);
    if (a.weight) {
        const float w = __uint_as_float(wbits);
        m = m && w >= a.w_lo && w < a.w_hi;  // false for NaN
    }
    return m;
}

template <bool kSrc>
using Tile = PairLoad<kSrc, kSelectThreads, kSelectUnroll, false>;  // one tile's loads; the odd record after them

// inclusive prefix sum over the 64 lanes of a wave
__device__ __forceinline__ uint32_t wave_scan(uint32_t v, uint32_t lane)
{
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

template <bool kSrc>
__global__ __launch_bounds__(kSelectThreads) void k_select_count(SelectArgs a)
{
    __shared__ uint32_t wave_tomb[kSelectThreads / 64];
    constexpr uint32_t U = kSelectUnroll;
    const uint32_t tid = threadIdx.x;
    uint32_t tomb = 0;
    for (uint64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const uint64_t first_pair = tile * (kSelectTile / 2);
        Tile<kSrc> t;
        t.load(a.s, first_pair, a.n, tid);
        uint32_t wave_matches = 0;  // wave-uniform
#pragma unroll
        for (uint32_t k = 0; k < U; ++k) {
            tomb += t.whole(k) ? (t.v[k].x == kAbsentDst) + (t.v[k].z == kAbsentDst) : 0u;
            const bool m0 = match<kSrc>(a, t.src0(k), t.v[k].x, t.v[k].y);
            const bool m1 = match<kSrc>(a, t.src1(k), t.v[k].z, t.v[k].w);
            wave_matches += __popcll(__ballot(m0)) + __popcll(__ballot(m1));
        }
        if ((tid & 63) == 0 && wave_matches) atomicAdd(a.counts + tile, wave_matches);
    }
    if ((a.n & 1) && blockIdx.x == 0 && tid == 0) {  // the last of the last tile
        const OddRecord r = odd_record<kSrc>(a.s, a.n);
        tomb += r.dst == kAbsentDst;
        if (match<kSrc>(a, r.src, r.dst, r.w)) atomicAdd(a.counts + (a.tiles - 1), 1u);
    }
    const uint32_t h[1] = {wave_add(tomb)};
    wave_words_to_lds(wave_tomb, h, tid);
    if (tid == 0) {
        unsigned long long s = 0;
        for (uint32_t w = 0; w < kSelectThreads / 64; ++w) s += wave_tomb[w];
        if (s) atomicAdd(a.out + 1, s);
    }
}

// Workgroup b scans segment b: kSelectScanSegment tiles, taken as kVec 16-B
// loads of four counts per thread; load j of thread t holds tiles 4 * (base +
// j * T + t) ..+3, so the prefix runs over (load, wave, lane, word).  It first
// sums every count before its segment itself (4 B per tile, from L2), so no
// workgroup waits for another.  The last workgroup writes the header.
__global__ __launch_bounds__(kSelectScanThreads) void k_select_scan(SelectArgs a)
{
    constexpr uint32_t T = kSelectScanThreads, W = T / 64, kVec = 4;
    static_assert(kVec * W == 64, "the (load, wave) totals are scanned by one wave, one per lane");
    static_assert(kVec * T * 4 == kSelectScanSegment, "a segment is kVec loads of four counts per thread");
    __shared__ uint32_t totals[kVec * W];
    __shared__ unsigned long long wave_before[W];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t vecs = (a.tiles + 3) >> 2;  // 16-B loads that hold a tile
    const u32x4* c4 = reinterpret_cast<const u32x4*>(a.counts);
    const uint64_t base = (uint64_t)blockIdx.x * (kVec * T);

    unsigned long long mine = 0;  // the matches before the segment: this thread's share
    for (uint64_t i = tid; i < base; i += kVec * T) {  // base is a multiple of kVec * T
        u32x4 c[kVec];
#pragma unroll
        for (uint32_t j = 0; j < kVec; ++j) c[j] = c4[i + j * T];
#pragma unroll
        for (uint32_t j = 0; j < kVec; ++j) mine += (unsigned long long)c[j].x + c[j].y + c[j].z + c[j].w;
    }
    for (int m = 32; m > 0; m >>= 1) mine += __shfl_xor(mine, m);
    if (lane == 0) wave_before[wave] = mine;

    u32x4 c[kVec];
    uint32_t incl[kVec];
#pragma unroll
    for (uint32_t j = 0; j < kVec; ++j) {
        const uint64_t i = base + j * T + tid;
        c[j] = i < vecs ? c4[i] : u32x4{0, 0, 0, 0};
    }
#pragma unroll
    for (uint32_t j = 0; j < kVec; ++j) {
        incl[j] = wave_scan(c[j].x + c[j].y + c[j].z + c[j].w, lane);
        if (lane == 63) totals[j * W + wave] = incl[j];
    }
    __syncthreads();
    unsigned long long carry = 0;
    for (uint32_t w = 0; w < W; ++w) carry += wave_before[w];
    const uint32_t before = wave_scan(totals[lane], lane);  // over the 64 (load, wave) totals
#pragma unroll
    for (uint32_t j = 0; j < kVec; ++j) {
        const uint64_t i = base + j * T + tid;
        const uint32_t e = j * W + wave;
        const uint32_t groups = e ? __shfl(before, e - 1) : 0u;
        if (i < vecs) {
            const unsigned long long o0 = carry + groups + (incl[j] - (c[j].x + c[j].y + c[j].z + c[j].w));
            const unsigned long long o1 = o0 + c[j].x, o2 = o1 + c[j].y, o3 = o2 + c[j].z;
            const uint64_t t = i << 2;  // tiles t .. t+3: the last load may hold fewer
            if (t + 3 < a.tiles) {
                u64x2* o = reinterpret_cast<u64x2*>(a.offsets + t);
                o[0] = u64x2{o0, o1};
                o[1] = u64x2{o2, o3};
            } else {
                a.offsets[t] = o0;
                if (t + 1 < a.tiles) a.offsets[t + 1] = o1;
                if (t + 2 < a.tiles) a.offsets[t + 2] = o2;
            }
        }
    }
    const unsigned long long matched = carry + __shfl(before, 63);
    if (blockIdx.x == gridDim.x - 1 && tid == 0) {
        a.out[0] = a.n;
        a.out[2] = matched;
        a.out[3] = matched < a.capacity ? matched : a.capacity;
        a.out[4] = a.syn_offset;
    }
}

template <bool kSrc>
__device__ __forceinline__ void emit_one(const SelectArgs& a, u32x4a8* rec, unsigned long long pos, uint64_t i, uint32_t src,
                                         uint32_t dst, uint32_t wbits)
{
    if (pos >= a.capacity) return;
    if (!kSrc) src = code_src(a.s.lo[i], a.s.hi[hi_pos(i)]);
    a.out[ABNN_SELECT_HEADER_WORDS + pos] = a.syn_offset + i;
    rec[pos] = u32x4a8{src, dst, wbits, 0u};
}

template <bool kSrc>
__global__ __launch_bounds__(kSelectThreads) void k_select_emit(SelectArgs a)
{
    constexpr uint32_t U = kSelectUnroll, W = kSelectThreads / 64;
    static_assert(U * W <= 64, "the (load, wave) totals are scanned by one wave");
    __shared__ uint32_t totals[2][U * W];
    __shared__ uint32_t list[kSelectEmitChunk];
    __shared__ uint32_t n_list;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    u32x4a8* rec = reinterpret_cast<u32x4a8*>(a.out + ABNN_SELECT_HEADER_WORDS + a.capacity);
    uint32_t parity = 0;
    // workgroup b looks at tiles b, b + G, b + 2G, ... (G workgroups), 64 of
    // them at once: neighbouring tiles, which tend to match together (the
    // generated graph's dense block), go to different workgroups
    const uint64_t G = gridDim.x;
    for (uint64_t chunk = 0; chunk * G + blockIdx.x < a.tiles; chunk += kSelectEmitChunk) {
        if (tid == 0) n_list = 0;
        __syncthreads();
        const uint64_t look = (chunk + tid) * G + blockIdx.x;
        if (tid < kSelectEmitChunk && look < a.tiles && a.counts[look] != 0 && a.offsets[look] < a.capacity)
            list[atomicAdd(&n_list, 1u)] = tid;  // in any order: a tile's output positions are its own
        __syncthreads();
        const uint32_t todo = n_list;
        for (uint32_t q = 0; q < todo; ++q, parity ^= 1) {
            const uint64_t tile = (chunk + list[q]) * G + blockIdx.x;
            const unsigned long long offset = a.offsets[tile];
            const uint64_t first_pair = tile * (kSelectTile / 2);
            Tile<kSrc> t;
            t.load(a.s, first_pair, a.n, tid);
            unsigned long long b0[U], b1[U];
            bool m0[U], m1[U];
#pragma unroll
            for (uint32_t k = 0; k < U; ++k) {
                m0[k] = match<kSrc>(a, t.src0(k), t.v[k].x, t.v[k].y);
                m1[k] = match<kSrc>(a, t.src1(k), t.v[k].z, t.v[k].w);
                b0[k] = __ballot(m0[k]);
                b1[k] = __ballot(m1[k]);
                if (lane == 0) totals[parity][k * W + wave] = __popcll(b0[k]) + __popcll(b1[k]);
            }
            __syncthreads();  // one per tile (the parity, as in k_select_scan)
            const uint32_t before = wave_scan(lane < U * W ? totals[parity][lane] : 0u, lane);
            const uint32_t in_pairs = __shfl(before, U * W - 1);  // the tile's matches inside 16-B pairs
            const unsigned long long below = (1ull << lane) - 1;
#pragma unroll
            for (uint32_t k = 0; k < U; ++k) {
                if (!(b0[k] | b1[k])) continue;  // wave-uniform
                const uint32_t e = k * W + wave;
                const uint32_t groups = e ? __shfl(before, e - 1) : 0u;
                const uint32_t r0 = groups + __popcll(b0[k] & below) + __popcll(b1[k] & below);
                const uint64_t i = t.pair(k) << 1;
                if (m0[k]) emit_one<kSrc>(a, rec, offset + r0, i, t.src0(k), t.v[k].x, t.v[k].y);
                if (m1[k]) emit_one<kSrc>(a, rec, offset + r0 + (m0[k] ? 1u : 0u), i + 1, t.src1(k), t.v[k].z, t.v[k].w);
            }
            if ((a.n & 1) && tile == a.tiles - 1 && tid == 0) {  // after every pair of the tile
                const OddRecord r = odd_record<kSrc>(a.s, a.n);
                if (match<kSrc>(a, r.src, r.dst, r.w)) emit_one<kSrc>(a, rec, offset + in_pairs, a.n - 1, r.src, r.dst, r.w);
            }
        }
        __syncthreads();  // list and n_list are rewritten by the next chunk
    }
}

}  // namespace

hipError_t launch_select(const SynArrays& syn, uint64_t n, uint64_t syn_offset, const abnn_select_config& cfg,
                         uint64_t capacity, const SelectScratch& scratch, uint64_t* out_dev, uint32_t blocks,
                         hipStream_t s)
{
    hipError_t e = hipMemsetAsync(out_dev, 0, ABNN_SELECT_HEADER_WORDS * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    SelectArgs a{};
    a.s = record_stream(syn);
    a.counts = scratch.counts;
    a.offsets = reinterpret_cast<unsigned long long*>(scratch.offsets);
    a.out = reinterpret_cast<unsigned long long*>(out_dev);
    a.n = n;
    a.tiles = select_tiles(n);
    a.capacity = capacity;
    a.syn_offset = syn_offset;
    a.any = (cfg.flags & ABNN_SELECT_ANY) ? 1u : 0u;
    a.weight = (cfg.flags & ABNN_SELECT_WEIGHT) ? 1u : 0u;
    const uint32_t unset = a.any ? 0u : 0xFFFFFFFFu;
    a.src_first = cfg.src_count ? cfg.src_first : 0u;
    a.src_span = cfg.src_count ? cfg.src_count : unset;
    a.dst_first = cfg.dst_count ? cfg.dst_first : 0u;
    a.dst_span = cfg.dst_count ? cfg.dst_count : unset;
    a.w_lo = cfg.w_lo;
    a.w_hi = cfg.w_hi;
    const bool src = cfg.src_count != 0;
    // grids from the CU count (capi.hip: 4 workgroups, 32 waves, per CU, as the census)
    const uint64_t resident = std::max(1u, blocks);
    if (n > 0) {
        e = hipMemsetAsync(scratch.counts, 0, select_count_words(n) * sizeof(uint32_t), s);
        if (e != hipSuccess) return e;
        const uint32_t grid = (uint32_t)std::min<uint64_t>(resident, a.tiles);
        if (src)
            hipLaunchKernelGGL(k_select_count<true>, dim3(grid), dim3(kSelectThreads), 0, s, a);
        else
            hipLaunchKernelGGL(k_select_count<false>, dim3(grid), dim3(kSelectThreads), 0, s, a);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const uint32_t segments = (uint32_t)std::max<uint64_t>(1, (a.tiles + kSelectScanSegment - 1) / kSelectScanSegment);
    hipLaunchKernelGGL(k_select_scan, dim3(segments), dim3(kSelectScanThreads), 0, s, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (n > 0 && capacity > 0) {
        const uint32_t grid = (uint32_t)std::min<uint64_t>(resident, a.tiles);
        if (src)
            hipLaunchKernelGGL(k_select_emit<true>, dim3(grid), dim3(kSelectThreads), 0, s, a);
        else
            hipLaunchKernelGGL(k_select_emit<false>, dim3(grid), dim3(kSelectThreads), 0, s, a);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace abnn
