// snapshot.hip -- the snapshot diff (abnn.h abnn_snapshot_diff_*, DESIGN.md
// §9): one streaming pass over two record arrays, `then` and `now`, that
// classifies every record pair below the shorter side's end and bins the weight
// changes.  The rule is snapshot.h diff_record, shared with the host function;
// every result word is an integer sum or maximum, so the result depends on
// neither the grid nor the order; abnn_amd/snapshot.py restates it in numpy.
//
//   k_diff : as k_census (census.hip).  Each lane loads 16 B = two {dst, w}
//       records from each side, and the two src streams of each side (4 B of lo
//       words, 2 B of hi bytes per pair and side): 22 B per record, every load
//       non-temporal (each side is read once), kDiffUnroll pairs in flight.
//       The class counts, net / abs and the maximum stay in registers; bins go
//       to a workgroup histogram in LDS kept in `copies` interleaved images
//       (census_copies' rule: hist[bin * copies + (lane & (copies - 1))]):
//       almost every d of a learning run falls into the one or two bins around
//       0, the census's constant-weight case.  The histogram is flushed once
//       per workgroup with global u64 atomics (zero bins skipped), then the
//       header: the waves reduce their counts, one atomic per word and
//       workgroup.  Workgroups are independent: no look-back, no ticket, no
//       residency assumption.
//   k_diff_finish : one thread, in stream order after it: words 0 .. 4.
//   k_src32_sync : the random-mode src mirror from the two src streams, after a
//       restore copied the streams over.
#include "snapshot.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace abnn {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kDiffLdsWords = 16384;  // 64 KiB of u32 counters per workgroup
constexpr uint32_t kDiffMaxCopies = 32;    // histogram copies, chosen by lane & (copies - 1)
constexpr uint32_t kDiffHead = 18;         // header sums per wave: words 5 .. 18, 21, net, abs, the maximum

// Histogram copies for `bins` bins: the most (a power of two, at most one per
// LDS bank) that fit the workgroup's counters.  4096 bins -> 4, <= 512 -> 32.
uint32_t diff_copies(uint32_t bins)
{
    uint32_t r = kDiffMaxCopies;
    while (r > 1 && (uint64_t)bins * r > kDiffLdsWords) r >>= 1;
    return r;
}

struct DiffSide {
    const u32x4* dw4;  // the {dst, w} stream, two records per element
    const uint2* dw;
    const uint16_t* lo;
    const uint8_t* hi;
};

struct DiffArgs {
    DiffSide a, b;  // then, now
    unsigned long long* out;
    uint64_t n;  // records compared: min(n_then, n_now)
    DiffRule rule;
    uint32_t copies;
};

__device__ __forceinline__ void diff_one(const DiffArgs& g, uint32_t* hist, uint32_t copy, uint32_t sa, uint32_t da,
                                         uint32_t wa, uint32_t sb, uint32_t db, uint32_t wb, DiffTally<uint32_t>& t)
{
    const uint32_t bin = diff_record(g.rule, sa, da, wa, sb, db, wb, t);
    if (bin != kDiffNoBin)
        __hip_atomic_fetch_add(&hist[bin * g.copies + copy], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ uint32_t wave_add(uint32_t v)
{
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
    for (int m = 32; m > 0; m >>= 1) {
        const uint32_t o = __shfl_xor(v, m);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ uint64_t wave_add64(uint64_t v)
{
    for (int m = 32; m > 0; m >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, m), hi = __shfl_xor((uint32_t)(v >> 32), m);
        v += (uint64_t)hi << 32 | lo;
    }
    return v;
}

__global__ __launch_bounds__(kDiffThreads) void k_diff(DiffArgs g)
{
    extern __shared__ uint32_t hist[];  // [bins * copies], at least 2 * kDiffHead words per wave
    constexpr uint32_t T = kDiffThreads, U = kDiffUnroll;
    const uint32_t tid = threadIdx.x;
    const uint32_t words = g.rule.bins * g.copies;
    for (uint32_t i = tid; i < words; i += T) hist[i] = 0;
    __syncthreads();

    const uint32_t copy = tid & (g.copies - 1);
    DiffTally<uint32_t> t;
    const uint64_t n_pairs = g.n >> 1;
    const uint64_t stride = (uint64_t)gridDim.x * (T * U);
    for (uint64_t base = (uint64_t)blockIdx.x * (T * U); base < n_pairs; base += stride) {
        u32x4 va[U], vb[U];
        uint32_t la[U], lb[U], ha[U], hb[U];
#pragma unroll
        for (uint32_t k = 0; k < U; ++k) {  // every load of the iteration before its first use
            const uint64_t p = base + k * T + tid;
            if (p < n_pairs) {
                va[k] = __builtin_nontemporal_load(g.a.dw4 + p);
                vb[k] = __builtin_nontemporal_load(g.b.dw4 + p);
                la[k] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(g.a.lo) + p);
                lb[k] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(g.b.lo) + p);
                ha[k] = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(g.a.hi) + p);
                hb[k] = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(g.b.hi) + p);
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < U; ++k) {
            const uint64_t p = base + k * T + tid;
            if (p < n_pairs) {
                diff_one(g, hist, copy, code_src(la[k] & 0xFFFFu, ha[k] & 0xFFu), va[k].x, va[k].y,
                         code_src(lb[k] & 0xFFFFu, hb[k] & 0xFFu), vb[k].x, vb[k].y, t);
                diff_one(g, hist, copy, code_src(la[k] >> 16, (ha[k] >> 8) & 0xFFu), va[k].z, va[k].w,
                         code_src(lb[k] >> 16, (hb[k] >> 8) & 0xFFu), vb[k].z, vb[k].w, t);
            }
        }
    }
    if ((g.n & 1) && blockIdx.x == 0 && tid == 0) {  // the record no pair holds
        const uint64_t i = g.n - 1;
        const uint2 ra = g.a.dw[i], rb = g.b.dw[i];
        diff_one(g, hist, copy, code_src(g.a.lo[i], g.a.hi[hi_pos(i)]), ra.x, ra.y,
                 code_src(g.b.lo[i], g.b.hi[hi_pos(i)]), rb.x, rb.y, t);
    }
    __syncthreads();

    // flush: a thread sums the copies of its bins, starting at its own copy so
    // that the lanes of a wave read different banks
    for (uint32_t b = tid; b < g.rule.bins; b += T) {
        uint32_t s = 0;
        for (uint32_t r = 0; r < g.copies; ++r) s += hist[b * g.copies + ((r + tid) & (g.copies - 1))];
        if (s) atomicAdd(g.out + ABNN_DIFF_HEADER_WORDS + b, (unsigned long long)s);
    }
    __syncthreads();  // the histogram is reused for the waves' header sums

    // the header: every wave's sums, then one atomic per word and workgroup
    uint64_t* s_head = reinterpret_cast<uint64_t*>(hist);  // [waves][kDiffHead]
    uint64_t h[kDiffHead];
#pragma unroll
    for (uint32_t j = 0; j < 14; ++j) h[j] = wave_add(t.count[j]);
    h[14] = wave_add(t.not_summable);
    h[15] = wave_add64((uint64_t)t.net);
    h[16] = wave_add64(t.abs);
    h[17] = wave_max(t.max_bits);
    if ((tid & 63) == 0) {
#pragma unroll
        for (uint32_t j = 0; j < kDiffHead; ++j) s_head[(tid >> 6) * kDiffHead + j] = h[j];
    }
    __syncthreads();
    if (tid < kDiffHead) {
        uint64_t s = 0;
        for (uint32_t w = 0; w < T / 64; ++w) {
            const uint64_t x = s_head[w * kDiffHead + tid];
            s = tid < 17 ? s + x : (x > s ? x : s);
        }
        // s_head column -> result word: 0 .. 13 -> 5 .. 18, 14 -> 21, 15 -> 19, 16 -> 20, 17 -> 22
        const uint32_t word = tid < 14 ? 5 + tid : tid == 14 ? 21 : tid == 15 ? 19 : tid == 16 ? 20 : 22;
        if (s) {
            if (tid < 17)
                atomicAdd(g.out + word, (unsigned long long)s);
            else
                atomicMax(g.out + word, (unsigned long long)s);
        }
    }
}

__global__ void k_diff_finish(unsigned long long* out, unsigned long long n_then, unsigned long long n_now)
{
    const unsigned long long c = n_then < n_now ? n_then : n_now;
    out[0] = n_now;
    out[1] = n_then;
    out[2] = c;
    out[3] = n_now - c;
    out[4] = n_then - c;
}

__global__ __launch_bounds__(256) void k_src32_sync(SynArrays a, uint64_t n)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
        a.src32[i] = code_src(a.lo[i], a.hi[hi_pos(i)]);
}

DiffSide side(const SynArrays& s)
{
    return DiffSide{reinterpret_cast<const u32x4*>(s.dw), s.dw, s.lo, s.hi};
}

}  // namespace

hipError_t launch_diff(const SynArrays& then, uint64_t n_then, const SynArrays& now, uint64_t n_now,
                       const DiffRule& rule, uint64_t* out_dev, uint32_t cus, hipStream_t s)
{
    const uint64_t words = ABNN_DIFF_HEADER_WORDS + (uint64_t)rule.bins;
    hipError_t e = hipMemsetAsync(out_dev, 0, words * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    unsigned long long* out = reinterpret_cast<unsigned long long*>(out_dev);
    const uint64_t n = std::min(n_then, n_now);
    if (n > 0) {
        DiffArgs g{};
        g.a = side(then);
        g.b = side(now);
        g.out = out;
        g.n = n;
        g.rule = rule;
        g.copies = diff_copies(rule.bins);
        const uint32_t lds_words = std::max<uint32_t>(g.rule.bins * g.copies, (kDiffThreads / 64) * 2 * kDiffHead);
        // grid from the CU count: as many workgroups per CU as their histograms
        // leave room for (160 KiB of LDS per CU), at most 4 (32 waves)
        const uint32_t per_cu = std::min<uint32_t>(4u, (160u * 1024u) / (lds_words * 4u));
        const uint64_t per_iter = 2ull * kDiffThreads * kDiffUnroll;  // records per workgroup iteration
        const uint64_t iters = (n + per_iter - 1) / per_iter;
        uint64_t grid = std::min<uint64_t>((uint64_t)std::max(1u, cus) * std::max(1u, per_cu), iters);
        // u32 LDS counters: no workgroup scans more than kDiffMaxPerWg records
        const uint64_t max_iters = kDiffMaxPerWg / per_iter;
        if ((iters + grid - 1) / grid > max_iters) grid = (iters + max_iters - 1) / max_iters;
        hipLaunchKernelGGL(k_diff, dim3((uint32_t)grid), dim3(kDiffThreads), lds_words * 4, s, g);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_diff_finish, dim3(1), dim3(1), 0, s, out, (unsigned long long)n_then,
                       (unsigned long long)n_now);
    return hipGetLastError();
}

hipError_t launch_src32_sync(const SynArrays& a, uint64_t n, hipStream_t s)
{
    if (n == 0 || !a.src32) return hipSuccess;
    hipLaunchKernelGGL(k_src32_sync, dim3((uint32_t)std::min<uint64_t>((n + 255) / 256, 4096)), dim3(256), 0, s, a, n);
    return hipGetLastError();
}

}  // namespace abnn
