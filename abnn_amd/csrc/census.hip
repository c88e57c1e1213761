// census.hip -- the synapse census (abnn.h abnn_census_*): one
// streaming pass over the local records [0, n_syn) that counts tombstones and
// bins the weights of the selected records.  Every result word is an integer
// count (or an order key's extreme), so the result does not depend on the
// grid, the order or the atomics; abnn_amd/census.py restates it in numpy.
//
//   k_census<kSrc> : the stream is scan.h's RecordStream, read by the kernel's
//       own loop (kCensusUnroll 16-B pair loads per lane and iteration; kSrc: a
//       src range is set), the odd last record by odd_record().  Header counts
//       and the min / max keys stay in registers; bin counts go to scan.h's
//       bank-spread histogram in LDS, flushed once with global u64 atomics,
//       then the header with one atomic per word and workgroup.  Workgroups
//       are independent: no look-back, no ticket, no residency assumption.
//   k_census_finish : one thread, in stream order after it: writes word 0 and
//       turns the two keys into f32 bits.
#include "census.h"
#include "scan.h"

#pragma clang fp contract(off)

namespace abnn {
namespace {

constexpr uint32_t kCensusHead = 7;  // header sums per wave (wave_words_to_lds packs them at this stride)

struct CensusArgs {
    RecordStream s;
    unsigned long long* out;
    uint64_t n;
    float w_lo, w_hi, scale;
    uint32_t bins, copies;
    // ranges as {first, span}: x is inside iff x - first < span (span = the
    // count, or 0xFFFFFFFF for "any": every live value passes)
    uint32_t src_first, src_span, dst_first, dst_span;
};

struct Tally {
    uint32_t tomb, sel, under, over, nan, kmin, kmax;
};

// the usual total order on f32 bits: negative values flip, others set the sign bit
__device__ __forceinline__ uint32_t order_key(uint32_t bits)
{
    return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

__device__ __forceinline__ uint32_t key_bits(uint32_t key)
{
    return key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu);
}

template <bool kSrc>
__device__ __forceinline__ void tally(const CensusArgs& a, uint32_t* hist, uint32_t copy, uint32_t src, uint32_t dst,
                                      uint32_t wbits, Tally& t)
{
    const bool tomb = dst == kAbsentDst;
    t.tomb += tomb ? 1u : 0u;
    bool sel = !tomb && dst - a.dst_first < a.dst_span;
    if (kSrc) sel = sel && src - a.src_first < a.src_span;
    if (!sel) return;
    t.sel += 1;
    const float w = __uint_as_float(wbits);
    if (w != w) {
        t.nan += 1;
        return;
    }
    const uint32_t key = order_key(wbits);
    t.kmin = key < t.kmin ? key : t.kmin;
    t.kmax = key > t.kmax ? key : t.kmax;
    if (w < a.w_lo) {
        t.under += 1;
        return;
    }
    if (w >= a.w_hi) {
        t.over += 1;
        return;
    }
    uint32_t bin = (uint32_t)((w - a.w_lo) * a.scale);
    bin = bin < a.bins - 1 ? bin : a.bins - 1;
    hist_add(hist, a.copies, copy, bin);
}

template <bool kSrc>
__global__ __launch_bounds__(kCensusThreads) void k_census(CensusArgs a)
{
    extern __shared__ uint32_t hist[];  // [bins * copies], at least kCensusHead words per wave
    constexpr uint32_t T = kCensusThreads, U = kCensusUnroll;
    const uint32_t tid = threadIdx.x;
    const uint32_t words = a.bins * a.copies;
    for (uint32_t i = tid; i < words; i += T) hist[i] = 0;
    __syncthreads();

    const uint32_t copy = tid & (a.copies - 1);
    Tally t{0, 0, 0, 0, 0, 0xFFFFFFFFu, 0u};
    const uint64_t n_pairs = a.n >> 1;  // whole pairs
    const uint64_t stride = (uint64_t)gridDim.x * (T * U);
    for (uint64_t base = (uint64_t)blockIdx.x * (T * U); base < n_pairs; base += stride) {
        // The loads stay written out here, not PairLoad's: with these, the
        // compiler lets a lane's loads wait for one another, and that is the
        // schedule the census's speed at four workgroups per CU rests on
        // (profiles/scan_refactor_ab.txt).  PairLoad keeps all U in flight:
        // another load policy.  A change of the record layout must be made
        // here and in k_diff (snapshot.hip) as well as in scan.h.
        u32x4 v[U];
        uint32_t lo2[U], hi2[U];
#pragma unroll
        for (uint32_t k = 0; k < U; ++k) {
            const uint64_t p = base + k * T + tid;
            if (p < n_pairs) {
                v[k] = __builtin_nontemporal_load(a.s.dw4 + p);
                if (kSrc) {
                    lo2[k] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(a.s.lo) + p);
                    hi2[k] = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(a.s.hi) + p);
                }
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < U; ++k) {
            const uint64_t p = base + k * T + tid;
            if (p < n_pairs) {
                uint32_t s0 = 0, s1 = 0;
                if (kSrc) {
                    s0 = code_src(lo2[k] & 0xFFFFu, hi2[k] & 0xFFu);
                    s1 = code_src(lo2[k] >> 16, (hi2[k] >> 8) & 0xFFu);
                }
                tally<kSrc>(a, hist, copy, s0, v[k].x, v[k].y, t);
                tally<kSrc>(a, hist, copy, s1, v[k].z, v[k].w, t);
            }
        }
    }
    if ((a.n & 1) && blockIdx.x == 0 && tid == 0) {
        const OddRecord r = odd_record<kSrc>(a.s, a.n);
        tally<kSrc>(a, hist, copy, r.src, r.dst, r.w, t);
    }
    __syncthreads();

    hist_flush(hist, a.bins, a.copies, tid, T, a.out + ABNN_CENSUS_HEADER_WORDS);
    __syncthreads();  // the histogram is reused for the waves' header sums

    // words 6 / 7 hold max(~min key) and max(max key) until k_census_finish:
    // both start at the zeros the buffer was cleared to
    const uint32_t h[kCensusHead] = {wave_add(t.tomb), wave_add(t.sel),   wave_add(t.under), wave_add(t.over),
                                     wave_add(t.nan),  wave_max(~t.kmin), wave_max(t.kmax)};
    wave_words_to_lds(hist, h, tid);
    if (tid < kCensusHead) {
        unsigned long long s = 0;
        for (uint32_t w = 0; w < T / 64; ++w) {
            const uint32_t x = hist[w * kCensusHead + tid];
            s = tid < 5 ? s + x : (x > s ? x : s);
        }
        if (s) {
            if (tid < 5)
                atomicAdd(a.out + 1 + tid, s);
            else
                atomicMax(a.out + 1 + tid, s);
        }
    }
}

__global__ void k_census_finish(unsigned long long* out, unsigned long long n)
{
    out[0] = n;
    const bool any = out[2] != out[5];  // a selected weight that is not NaN
    const uint32_t kmin = ~(uint32_t)out[6], kmax = (uint32_t)out[7];
    out[6] = any ? key_bits(kmin) : 0x7F800000u;  // +inf
    out[7] = any ? key_bits(kmax) : 0xFF800000u;  // -inf
}

}  // namespace

hipError_t launch_census(const SynArrays& syn, uint64_t n, const abnn_census_config& cfg, float scale,
                         uint64_t* out_dev, uint32_t cus, hipStream_t s)
{
    const uint64_t words = ABNN_CENSUS_HEADER_WORDS + (uint64_t)cfg.bins;
    hipError_t e = hipMemsetAsync(out_dev, 0, words * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    unsigned long long* out = reinterpret_cast<unsigned long long*>(out_dev);
    if (n > 0) {
        CensusArgs a{};
        a.s = record_stream(syn);
        a.out = out;
        a.n = n;
        a.w_lo = cfg.lo;
        a.w_hi = cfg.hi;
        a.scale = scale;
        a.bins = cfg.bins;
        a.copies = hist_copies(cfg.bins);
        a.src_first = cfg.src_first;
        a.src_span = cfg.src_count ? cfg.src_count : 0xFFFFFFFFu;
        a.dst_first = cfg.dst_count ? cfg.dst_first : 0u;
        a.dst_span = cfg.dst_count ? cfg.dst_count : 0xFFFFFFFFu;
        const uint32_t lds_words = std::max<uint32_t>(a.bins * a.copies, (kCensusThreads / 64) * kCensusHead);
        const uint32_t grid = scan_grid(n, 2ull * kCensusThreads * kCensusUnroll, lds_words, cus, kScanMaxPerWg);
        if (cfg.src_count)
            hipLaunchKernelGGL(k_census<true>, dim3(grid), dim3(kCensusThreads), lds_words * 4, s, a);
        else
            hipLaunchKernelGGL(k_census<false>, dim3(grid), dim3(kCensusThreads), lds_words * 4, s, a);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_census_finish, dim3(1), dim3(1), 0, s, out, (unsigned long long)n);
    return hipGetLastError();
}

}  // namespace abnn
