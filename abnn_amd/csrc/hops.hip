// hops.hip -- reachability (abnn.h abnn_hops_*): the hop distance
// of every neuron from a seed set, a breadth-first search whose every hop is one
// streaming pass over the local records [0, n_syn) against a one-bit-per-neuron
// frontier map (N_NRN / 8 bytes: it stays in the L2).  Distances are
// breadth-first levels and the only write to the plane is an atomic minimum, so
// the result does not depend on the grid, the order or the timing;
// abnn_amd/hops.py restates it in numpy.
//
//   k_hops_begin     : header and levels zero, plane = 0 on the seeds and
//                      UNREACHED elsewhere (8-B stores).
//   k_hops_frontier  : step h.  Reads the plane with 16-B loads (four neurons
//                      per lane), ORs eight lanes' nibbles into one bitmap word
//                      and writes EVERY word of the bitmap (no memset), counts
//                      plane[n] == h into levels[h] with one atomic per
//                      workgroup.  Returns at once when levels[h-1] == 0.
//   k_hops_expand<kReverse, kWeight> : step h < H.  Returns at once when
//                      levels[h] == 0.  Workgroups are independent: no
//                      look-back, no ticket, no residency assumption.
//       forward: streams lo[] and hi[] only (3 B per record), non-temporal,
//         16 B of lo and 8 B of hi = eight records per lane and load, every
//         load of an iteration issued before its first use; decodes the src,
//         tests its frontier bit (the eight bitmap gathers issued together),
//         and only for a hit gathers dw[k].
//       reverse: the stream is scan.h's, without the src streams; tests the
//         bit of dst, and only for a hit reads lo[k] and hi[k].
//       The records that no whole forward load holds (n_syn % 8) are read one
//       at a time by one thread: nothing is read past record n_syn - 1.
//       A hit that is live, in bounds and inside the weight interval issues
//       atomicMin(plane[v], h + 1) (agent scope, relaxed, no return).  The plain
//       read of plane[v] before it only skips the atomic for a neuron that is
//       already set: a stale value can only be LARGER than the true one (the
//       plane only decreases), so a skip is always right, and correctness rests
//       on the atomic alone.
//   k_hops_close     : one workgroup, header words 0..4 from the levels.
#include "hops.h"
#include "scan.h"

#pragma clang fp contract(off)

namespace abnn {
namespace {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned long long u64;

constexpr uint32_t kUnreached = ABNN_HOPS_UNREACHED;
static_assert(kUnreached == kAbsentDst, "the reverse pass: an absent record is one whose dst is no neuron");

struct HopsArgs {
    const uint16_t* lo;
    const uint8_t* hi;
    const uint2* dw;
    u64* out;                // header | levels[0..H] | plane
    const uint32_t* bitmap;  // the frontier of step h
    uint64_t n;              // records
    uint32_t n_nrn, H, h;
    float w_lo, w_hi;
};

__device__ __forceinline__ u64* levels_of(u64* out) { return out + ABNN_HOPS_HEADER_WORDS; }
__device__ __forceinline__ uint32_t* plane_of(u64* out, uint32_t H)
{
    return reinterpret_cast<uint32_t*>(out + ABNN_HOPS_HEADER_WORDS + H + 1);
}

__global__ __launch_bounds__(kHopsFrontierThreads) void k_hops_begin(u64* out, uint32_t H, uint32_t n_nrn, uint32_t first,
                                                                     uint32_t count)
{
    const uint32_t tid = threadIdx.x;
    if (blockIdx.x == 0)
        for (uint32_t j = tid; j < ABNN_HOPS_HEADER_WORDS + H + 1; j += kHopsFrontierThreads) out[j] = 0;
    u32x2* plane2 = reinterpret_cast<u32x2*>(out + ABNN_HOPS_HEADER_WORDS + H + 1);
    const uint32_t n_words = (uint32_t)(((uint64_t)n_nrn + 1) >> 1);
    for (uint32_t j = blockIdx.x * kHopsFrontierThreads + tid; j < n_words; j += gridDim.x * kHopsFrontierThreads) {
        const uint32_t n0 = 2 * j, n1 = 2 * j + 1;  // n1 == n_nrn: the pad entry of an odd N_NRN, 0
        u32x2 v;
        v.x = (n0 - first < count) ? 0u : kUnreached;
        v.y = (n1 >= n_nrn || n1 - first < count) ? 0u : kUnreached;
        plane2[j] = v;
    }
}

__global__ __launch_bounds__(kHopsFrontierThreads) void k_hops_frontier(u64* out, uint32_t* bitmap, uint32_t H, uint32_t n_nrn,
                                                                        uint32_t h)
{
    __shared__ uint32_t sums[kHopsFrontierThreads / 64];
    constexpr uint32_t T = kHopsFrontierThreads;
    u64* levels = levels_of(out);
    if (h > 0 && __hip_atomic_load(levels + h - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
    const uint32_t* plane = plane_of(out, H);
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    // one 16-B vector = four neurons per lane, eight lanes = one bitmap word;
    // whole groups of eight lanes, so that every word is written
    const uint32_t n_vec = (uint32_t)((((uint64_t)n_nrn + 31) >> 5) << 3);
    uint32_t count = 0;
    // uniform over the wave: a lane past the end carries an empty nibble through the shuffles
    for (uint32_t base = blockIdx.x * T; base < n_vec; base += gridDim.x * T) {
        const uint32_t v = base + tid;
        const uint64_t at = 4ull * v;
        uint32_t nib = 0;
        if (at + 4 <= n_nrn) {
            u32x4 x;  // the plane is 8-byte aligned (an even or odd H + 1 words behind the header)
            __builtin_memcpy(&x, plane + at, 16);
            nib = (x.x == h ? 1u : 0u) | (x.y == h ? 2u : 0u) | (x.z == h ? 4u : 0u) | (x.w == h ? 8u : 0u);
        } else {
            for (uint32_t c = 0; c < 4; ++c)
                if (at + c < n_nrn && plane[at + c] == h) nib |= 1u << c;
        }
        count += __popc(nib);
        uint32_t w = nib << (4u * (lane & 7u));
        w |= __shfl_xor(w, 1);
        w |= __shfl_xor(w, 2);
        w |= __shfl_xor(w, 4);
        if ((lane & 7u) == 0 && v < n_vec) bitmap[v >> 3] = w;
    }
    count = wave_add(count);
    if (lane == 0) sums[tid >> 6] = count;
    __syncthreads();
    if (tid == 0) {
        uint32_t s = 0;
        for (uint32_t w = 0; w < T / 64; ++w) s += sums[w];
        if (s) __hip_atomic_fetch_add(levels + h, (u64)s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The bitmap word of neuron n, 0 when n cannot be in the frontier.  The load is
// issued whether or not n is a neuron (n >= N_NRN: the tombstone's src code, a
// tombstone's dst, a record that was never validated -- word 0 then), so that a
// lane's gathers are all issued before the first one is used.  With the fold
// (k_hops_expand) a neuron whose folded bit is clear loads word 0 as well: the
// lanes of a wave that miss share one cache line.
__device__ __forceinline__ uint32_t frontier_word(const HopsArgs& a, const uint32_t* fold, bool use_fold, uint32_t n)
{
    bool may = n < a.n_nrn;
    if (use_fold) may = may && ((fold[(n >> 5) & (kHopsFoldWords - 1u)] >> (n & 31u)) & 1u);
    const uint32_t w = a.bitmap[may ? n >> 5 : 0u];
    return may ? w : 0u;
}

__device__ __forceinline__ bool in_frontier(const HopsArgs& a, uint32_t n, uint32_t word)
{
    return n < a.n_nrn && ((word >> (n & 31u)) & 1u);
}

__device__ __forceinline__ void relax(const HopsArgs& a, uint32_t* plane, uint32_t v)
{
    if (plane[v] <= a.h + 1u) return;  // a hint only (see the head of this file)
    (void)__hip_atomic_fetch_min(plane + v, a.h + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool kWeight>
__device__ __forceinline__ bool weight_ok(const HopsArgs& a, uint32_t wbits)
{
    if (!kWeight) return true;
    const float w = __uint_as_float(wbits);
    return w >= a.w_lo && w < a.w_hi;  // false for NaN
}

// Forward: `count` (<= 8) records from record `first` on, their src codes packed
// as the streams hold them (lo: 2 B each, hi: 1 B each).  A hit gathers dw[k].
template <bool kWeight>
__device__ __forceinline__ void forward_group(const HopsArgs& a, const uint32_t* fold, bool use_fold, uint32_t* plane,
                                              uint64_t first, uint32_t count, const uint32_t (&lw)[4],
                                              const uint32_t (&hw)[2])
{
    uint32_t src[8], word[8];
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
        src[j] = code_src((lw[j >> 1] >> (16u * (j & 1u))) & 0xFFFFu, (hw[j >> 2] >> (8u * (j & 3u))) & 0xFFu);
        word[j] = frontier_word(a, fold, use_fold, src[j]);
    }
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
        if (j < count && in_frontier(a, src[j], word[j])) {
            const uint2 r = a.dw[first + j];
            // a tombstone's dst is above N_NRN
            if (r.x < a.n_nrn && weight_ok<kWeight>(a, r.y)) relax(a, plane, r.x);
        }
    }
}

// Reverse: record k = {dst, w}; a hit reads the record's src code.
template <bool kWeight>
__device__ __forceinline__ void reverse_record(const HopsArgs& a, uint32_t* plane, uint64_t k, uint32_t dst, uint32_t wbits,
                                               uint32_t word)
{
    if (!in_frontier(a, dst, word) || !weight_ok<kWeight>(a, wbits)) return;
    const uint32_t src = code_src(a.lo[k], a.hi[hi_pos(k)]);
    if (src < a.n_nrn) relax(a, plane, src);
}

template <bool kReverse, bool kWeight>
__global__ __launch_bounds__(kHopsThreads) void k_hops_expand(HopsArgs a)
{
    __shared__ uint32_t fold[kHopsFoldWords];
    constexpr uint32_t T = kHopsThreads;
    const u64 frontier = __hip_atomic_load(levels_of(a.out) + a.h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (frontier == 0) return;
    uint32_t* plane = plane_of(a.out, a.H);
    const uint32_t tid = threadIdx.x;
    // A sparse frontier: the bitmap folded to kHopsFoldWords words in LDS (word w
    // ORed into word w mod kHopsFoldWords) rejects nearly every record without a
    // gather from the L2; a record that passes is confirmed against the bitmap.
    // A bitmap that fits is held whole.  Uniform over the grid.
    const uint32_t bm_words = (uint32_t)(((uint64_t)a.n_nrn + 31) >> 5);  // hops_bitmap_words
    const bool use_fold = frontier <= kHopsFoldMaxFrontier || bm_words <= kHopsFoldWords;
    if (use_fold) {
        for (uint32_t i = tid; i < kHopsFoldWords; i += T) {
            uint32_t w = 0;
            for (uint32_t j = i; j < bm_words; j += kHopsFoldWords) w |= a.bitmap[j];
            fold[i] = w;
        }
        __syncthreads();
    }
    if (!kReverse) {
        constexpr uint32_t U = kHopsFwdUnroll;
        const u32x4* lo4 = reinterpret_cast<const u32x4*>(a.lo);
        const u32x2* hi2 = reinterpret_cast<const u32x2*>(a.hi);
        const uint64_t n_groups = a.n >> 3;  // whole groups of eight records
        const uint64_t stride = (uint64_t)gridDim.x * (T * U);
        for (uint64_t base = (uint64_t)blockIdx.x * (T * U); base < n_groups; base += stride) {
            u32x4 l[U];
            u32x2 hh[U];
#pragma unroll
            for (uint32_t k = 0; k < U; ++k) {  // every load of the iteration before its first use
                const uint64_t g = base + k * T + tid;
                l[k] = u32x4{0u, 0u, 0u, 0u};
                hh[k] = u32x2{0u, 0u};
                if (g < n_groups) {
                    l[k] = __builtin_nontemporal_load(lo4 + g);
                    hh[k] = __builtin_nontemporal_load(hi2 + g);
                }
            }
#pragma unroll
            for (uint32_t k = 0; k < U; ++k) {
                const uint64_t g = base + k * T + tid;
                const uint32_t lw[4] = {l[k].x, l[k].y, l[k].z, l[k].w}, hw[2] = {hh[k].x, hh[k].y};
                forward_group<kWeight>(a, fold, use_fold, plane, 8 * g, g < n_groups ? 8u : 0u, lw, hw);
            }
        }
        // the records no whole group holds, one at a time: nothing is read past record n - 1
        const uint32_t rest = (uint32_t)(a.n & 7u);
        if (rest && blockIdx.x == 0 && tid == 0) {
            uint32_t lw[4] = {0, 0, 0, 0}, hw[2] = {0, 0};
            for (uint32_t j = 0; j < rest; ++j) {
                const uint64_t k = 8 * n_groups + j;
                lw[j >> 1] |= (uint32_t)a.lo[k] << (16u * (j & 1u));
                hw[j >> 2] |= (uint32_t)a.hi[hi_pos(k)] << (8u * (j & 3u));
            }
            forward_group<kWeight>(a, fold, use_fold, plane, 8 * n_groups, rest, lw, hw);
        }
    } else {
        constexpr uint32_t U = kHopsRevUnroll;
        const RecordStream rs{reinterpret_cast<const u32x4*>(a.dw), a.dw, a.lo, a.hi};
        const uint64_t n_pairs = scan_pairs(a.n);
        const uint64_t stride = (uint64_t)gridDim.x * (T * U);
        for (uint64_t base = (uint64_t)blockIdx.x * (T * U); base < n_pairs; base += stride) {
            PairLoad<false, T, U> l;  // an absent record: a dst above N_NRN
            l.load(rs, base, a.n, tid);
            uint32_t w0[U], w1[U];
#pragma unroll
            for (uint32_t k = 0; k < U; ++k) {
                w0[k] = frontier_word(a, fold, use_fold, l.v[k].x);
                w1[k] = frontier_word(a, fold, use_fold, l.v[k].z);
            }
#pragma unroll
            for (uint32_t k = 0; k < U; ++k) {
                const uint64_t p = l.pair(k);
                reverse_record<kWeight>(a, plane, 2 * p, l.v[k].x, l.v[k].y, w0[k]);
                reverse_record<kWeight>(a, plane, 2 * p + 1, l.v[k].z, l.v[k].w, w1[k]);
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_hops_close(u64* out, uint32_t H, uint64_t n, uint32_t n_nrn)
{
    __shared__ u64 s_sum[256];
    __shared__ uint32_t s_depth[256];
    const u64* levels = levels_of(out);
    const uint32_t tid = threadIdx.x;
    u64 sum = 0;
    uint32_t depth = 0;
    for (uint32_t j = tid; j <= H; j += 256) {
        const u64 c = levels[j];
        sum += c;
        if (c) depth = j;  // j increases
    }
    s_sum[tid] = sum;
    s_depth[tid] = depth;
    __syncthreads();
    if (tid == 0) {
        for (uint32_t t = 1; t < 256; ++t) {
            sum += s_sum[t];
            depth = depth > s_depth[t] ? depth : s_depth[t];
        }
        out[0] = n;
        out[1] = n_nrn;
        out[2] = sum;
        out[3] = depth;
        out[4] = levels[H] == 0 ? 1u : 0u;
    }
}

}  // namespace

hipError_t launch_hops_step(const SynArrays& syn, uint64_t n, const abnn_hops_config& cfg, uint64_t n_nrn, uint32_t step,
                            uint64_t* out_dev, uint32_t* bitmap, uint32_t cus, hipStream_t s)
{
    u64* out = reinterpret_cast<u64*>(out_dev);
    const uint32_t H = cfg.max_hops, nn = (uint32_t)n_nrn;
    cus = std::max(1u, cus);
    constexpr uint32_t FT = kHopsFrontierThreads;
    if (step == ABNN_HOPS_BEGIN) {
        const uint64_t blocks = std::min<uint64_t>(8ull * cus, ((n_nrn + 1) / 2 + FT - 1) / FT);
        hipLaunchKernelGGL(k_hops_begin, dim3((uint32_t)std::max<uint64_t>(1, blocks)), dim3(FT), 0, s, out, H, nn,
                           cfg.seed_first, cfg.seed_count);
        return hipGetLastError();
    }
    {
        const uint64_t vecs = hops_bitmap_words(n_nrn) * 8;
        const uint64_t blocks = std::min<uint64_t>(8ull * cus, (vecs + FT - 1) / FT);
        hipLaunchKernelGGL(k_hops_frontier, dim3((uint32_t)std::max<uint64_t>(1, blocks)), dim3(FT), 0, s, out, bitmap, H, nn,
                           step);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (step == H) {
        hipLaunchKernelGGL(k_hops_close, dim3(1), dim3(256), 0, s, out, H, (uint64_t)n, nn);
        return hipGetLastError();
    }
    if (n == 0) return hipSuccess;
    HopsArgs a{};
    a.lo = syn.lo;
    a.hi = syn.hi;
    a.dw = syn.dw;
    a.out = out;
    a.bitmap = bitmap;
    a.n = n;
    a.n_nrn = nn;
    a.H = H;
    a.h = step;
    a.w_lo = cfg.w_lo;
    a.w_hi = cfg.w_hi;
    const bool rev = cfg.flags & ABNN_HOPS_REVERSE, wt = cfg.flags & ABNN_HOPS_WEIGHT;
    // records per workgroup iteration; 4 workgroups (32 waves) per CU, as the census.  At least one
    // workgroup: forward, its first thread takes the records that no whole load holds.
    const uint64_t per_iter = rev ? 2ull * kHopsThreads * kHopsRevUnroll : 8ull * kHopsThreads * kHopsFwdUnroll;
    const uint64_t iters = (n + per_iter - 1) / per_iter;
    const dim3 g((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(4ull * cus, iters))), b(kHopsThreads);
    if (rev && wt)
        hipLaunchKernelGGL((k_hops_expand<true, true>), g, b, 0, s, a);
    else if (rev)
        hipLaunchKernelGGL((k_hops_expand<true, false>), g, b, 0, s, a);
    else if (wt)
        hipLaunchKernelGGL((k_hops_expand<false, true>), g, b, 0, s, a);
    else
        hipLaunchKernelGGL((k_hops_expand<false, false>), g, b, 0, s, a);
    return hipGetLastError();
}

}  // namespace abnn
