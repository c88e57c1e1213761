// snapshot.hip -- the snapshot diff (abnn.h abnn_snapshot_diff_*, DESIGN.md
// §9): one streaming pass over two record arrays, `then` and `now`, that
// classifies every record pair below the shorter side's end and bins the weight
// changes.  The rule is snapshot.h diff_record, shared with the host function;
// every result word is an integer sum or maximum, so the result depends on
// neither the grid nor the order; abnn_amd/snapshot.py restates it in numpy.
//
//   k_diff : as k_census (census.hip): scan.h's RecordStream once per side,
//       read by the kernel's own loop with both src streams (22 B per record,
//       kDiffUnroll pairs per lane and iteration), the odd last record by
//       odd_record().  The class counts, net / abs and the maximum stay in registers;
//       bins go to scan.h's bank-spread histogram in LDS: almost every d of a
//       learning run falls into the one or two bins around 0, the census's
//       constant-weight case.  The histogram is flushed once per workgroup
//       with global u64 atomics, then the header: one atomic per word and
//       workgroup.  Workgroups are independent: no look-back, no ticket, no
//       residency assumption.
//   k_diff_finish : one thread, in stream order after it: words 0 .. 4.
//   k_src32_sync : the random-mode src mirror from the two src streams, after a
//       restore copied the streams over.
#include "snapshot.h"
#include "scan.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace abnn {
namespace {

constexpr uint32_t kDiffHead = 18;  // header sums per wave: words 5 .. 18, 21, net, abs, the maximum

struct DiffArgs {
    RecordStream a, b;  // then, now
    unsigned long long* out;
    uint64_t n;  // records compared: min(n_then, n_now)
    DiffRule rule;
    uint32_t copies;
};

__device__ __forceinline__ void diff_one(const DiffArgs& g, uint32_t* hist, uint32_t copy, uint32_t sa, uint32_t da,
                                         uint32_t wa, uint32_t sb, uint32_t db, uint32_t wb, DiffTally<uint32_t>& t)
{
    const uint32_t bin = diff_record(g.rule, sa, da, wa, sb, db, wb, t);
    if (bin != kDiffNoBin) hist_add(hist, g.copies, copy, bin);
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
    const uint64_t n_pairs = g.n >> 1;  // whole pairs
    const uint64_t stride = (uint64_t)gridDim.x * (T * U);
    for (uint64_t base = (uint64_t)blockIdx.x * (T * U); base < n_pairs; base += stride) {
        // The loads stay written out here, not PairLoad's, as in k_census and
        // for its reason: the diff's speed rests on the schedule the compiler
        // gives this loop (profiles/scan_refactor_ab.txt).  A change of the
        // record layout must be made here and in k_census (census.hip) as
        // well as in scan.h.
        u32x4 va[U], vb[U];
        uint32_t la[U], lb[U], ha[U], hb[U];
#pragma unroll
        for (uint32_t k = 0; k < U; ++k) {
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
    if ((g.n & 1) && blockIdx.x == 0 && tid == 0) {
        const OddRecord ra = odd_record<true>(g.a, g.n), rb = odd_record<true>(g.b, g.n);
        diff_one(g, hist, copy, ra.src, ra.dst, ra.w, rb.src, rb.dst, rb.w, t);
    }
    __syncthreads();

    hist_flush(hist, g.rule.bins, g.copies, tid, T, g.out + ABNN_DIFF_HEADER_WORDS);
    __syncthreads();  // the histogram is reused for the waves' header sums

    // the header: every wave's sums, then one atomic per word and workgroup
    uint64_t* s_head = reinterpret_cast<uint64_t*>(hist);  // [waves][kDiffHead]
    uint64_t h[kDiffHead];
#pragma unroll
    for (uint32_t j = 0; j < 14; ++j) h[j] = wave_add(t.count[j]);
    h[14] = wave_add(t.not_summable);
    h[15] = wave_add((uint64_t)t.net);
    h[16] = wave_add(t.abs);
    h[17] = wave_max(t.max_bits);
    wave_words_to_lds(s_head, h, tid);
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
        g.a = record_stream(then);
        g.b = record_stream(now);
        g.out = out;
        g.n = n;
        g.rule = rule;
        g.copies = hist_copies(rule.bins);
        const uint32_t lds_words = std::max<uint32_t>(g.rule.bins * g.copies, (kDiffThreads / 64) * 2 * kDiffHead);
        const uint32_t grid = scan_grid(n, 2ull * kDiffThreads * kDiffUnroll, lds_words, cus, kScanMaxPerWg);
        hipLaunchKernelGGL(k_diff, dim3(grid), dim3(kDiffThreads), lds_words * 4, s, g);
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
