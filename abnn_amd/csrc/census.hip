// census.hip -- the synapse census (abnn.h abnn_census_*): one
// streaming pass over the local records [0, n_syn) that counts tombstones and
// bins the weights of the selected records.  Every result word is an integer
// count (or an order key's extreme), so the result does not depend on the
// grid, the order or the atomics; abnn_amd/census.py restates it in numpy.
//
//   k_census<kSrc> : each lane loads 16 B = two {dst, w} records at a time
//       (kCensusUnroll loads in flight), non-temporal: the records are read
//       once.  Only the kSrc instantiation (a src range is set) reads the two
//       src streams.  Header counts and the min / max keys stay in registers;
//       bin counts go to a workgroup histogram in LDS, flushed once with global
//       u64 atomics (zero bins skipped), then the header with one atomic per
//       word and workgroup.  Workgroups are independent: no look-back, no
//       ticket, no residency assumption.
//   k_census_finish : one thread, in stream order after it: writes word 0 and
//       turns the two keys into f32 bits.
//
// Contention.  A weight distribution that falls into a few bins (the generated
// graph: 6-7 of 64; a constant weight: one) would serialise a single LDS
// histogram on those addresses.  The workgroup therefore keeps `copies`
// histograms (census_copies: 32 up to 512 bins, 4 at 4096), interleaved as
// hist[bin * copies + (lane & (copies - 1))]: with 32 copies the 32 lanes an
// LDS atomic services together always hit 32 different banks, whatever their
// bins are; with fewer, equal bins from different lanes still spread over
// `copies` banks (a constant weight at 4096 bins: 8 lanes per address).
#include "census.h"

#pragma clang fp contract(off)

namespace abnn {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct CensusArgs {
    const u32x4* dw4;  // the {dst, w} stream, two records per element
    const uint2* dw;
    const uint16_t* lo;
    const uint8_t* hi;
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
    const bool tomb = dst == 0xFFFFFFFFu;
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
    __hip_atomic_fetch_add(&hist[bin * a.copies + copy], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
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

template <bool kSrc>
__global__ __launch_bounds__(kCensusThreads) void k_census(CensusArgs a)
{
    extern __shared__ uint32_t hist[];  // [bins * copies], at least 8 words per wave
    constexpr uint32_t T = kCensusThreads, U = kCensusUnroll;
    const uint32_t tid = threadIdx.x;
    const uint32_t words = a.bins * a.copies;
    for (uint32_t i = tid; i < words; i += T) hist[i] = 0;
    __syncthreads();

    const uint32_t copy = tid & (a.copies - 1);
    Tally t{0, 0, 0, 0, 0, 0xFFFFFFFFu, 0u};
    const uint64_t n_pairs = a.n >> 1;
    const uint64_t stride = (uint64_t)gridDim.x * (T * U);
    for (uint64_t base = (uint64_t)blockIdx.x * (T * U); base < n_pairs; base += stride) {
        u32x4 v[U];
        uint32_t lo2[U], hi2[U];
#pragma unroll
        for (uint32_t k = 0; k < U; ++k) {  // every load of the iteration before its first use
            const uint64_t p = base + k * T + tid;
            if (p < n_pairs) {
                v[k] = __builtin_nontemporal_load(a.dw4 + p);
                if (kSrc) {
                    lo2[k] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(a.lo) + p);
                    hi2[k] = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(a.hi) + p);
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
    if ((a.n & 1) && blockIdx.x == 0 && tid == 0) {  // the record no pair holds
        const uint64_t i = a.n - 1;
        const uint2 r = a.dw[i];
        tally<kSrc>(a, hist, copy, kSrc ? code_src(a.lo[i], a.hi[hi_pos(i)]) : 0u, r.x, r.y, t);
    }
    __syncthreads();

    // flush: a thread sums the copies of its bins, starting at its own copy so
    // that the lanes of a wave read different banks
    for (uint32_t b = tid; b < a.bins; b += T) {
        uint32_t s = 0;
        for (uint32_t r = 0; r < a.copies; ++r) s += hist[b * a.copies + ((r + tid) & (a.copies - 1))];
        if (s) atomicAdd(a.out + ABNN_CENSUS_HEADER_WORDS + b, (unsigned long long)s);
    }
    __syncthreads();  // the histogram is reused for the waves' header sums

    // words 6 / 7 hold max(~min key) and max(max key) until k_census_finish:
    // both start at the zeros the buffer was cleared to
    const uint32_t h[7] = {wave_add(t.tomb), wave_add(t.sel),   wave_add(t.under), wave_add(t.over),
                           wave_add(t.nan),  wave_max(~t.kmin), wave_max(t.kmax)};
    if ((tid & 63) == 0)
        for (uint32_t j = 0; j < 7; ++j) hist[(tid >> 6) * 8 + j] = h[j];
    __syncthreads();
    if (tid < 7) {
        unsigned long long s = 0;
        for (uint32_t w = 0; w < T / 64; ++w) {
            const uint32_t x = hist[w * 8 + tid];
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
        a.dw4 = reinterpret_cast<const u32x4*>(syn.dw);
        a.dw = syn.dw;
        a.lo = syn.lo;
        a.hi = syn.hi;
        a.out = out;
        a.n = n;
        a.w_lo = cfg.lo;
        a.w_hi = cfg.hi;
        a.scale = scale;
        a.bins = cfg.bins;
        a.copies = census_copies(cfg.bins);
        a.src_first = cfg.src_first;
        a.src_span = cfg.src_count ? cfg.src_count : 0xFFFFFFFFu;
        a.dst_first = cfg.dst_count ? cfg.dst_first : 0u;
        a.dst_span = cfg.dst_count ? cfg.dst_count : 0xFFFFFFFFu;
        const uint32_t lds_words = std::max<uint32_t>(a.bins * a.copies, (kCensusThreads / 64) * 8);
        // grid from the CU count: as many workgroups per CU as their histograms
        // leave room for (160 KiB of LDS per CU), at most 4 (32 waves)
        const uint32_t per_cu = std::min<uint32_t>(4u, (160u * 1024u) / (lds_words * 4u));
        const uint64_t per_iter = 2ull * kCensusThreads * kCensusUnroll;  // records per workgroup iteration
        const uint64_t iters = (n + per_iter - 1) / per_iter;
        uint64_t grid = std::min<uint64_t>((uint64_t)std::max(1u, cus) * per_cu, iters);
        // u32 LDS counters: no workgroup scans more than kCensusMaxPerWg records
        const uint64_t max_iters = kCensusMaxPerWg / per_iter;
        if ((iters + grid - 1) / grid > max_iters) grid = (iters + max_iters - 1) / max_iters;
        if (cfg.src_count)
            hipLaunchKernelGGL(k_census<true>, dim3((uint32_t)grid), dim3(kCensusThreads), lds_words * 4, s, a);
        else
            hipLaunchKernelGGL(k_census<false>, dim3((uint32_t)grid), dim3(kCensusThreads), lds_words * 4, s, a);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_census_finish, dim3(1), dim3(1), 0, s, out, (unsigned long long)n);
    return hipGetLastError();
}

}  // namespace abnn
