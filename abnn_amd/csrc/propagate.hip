// propagate.hip -- signal propagation (abnn.h abnn_propagate_*):
// one streaming pass over the local records [0, n_syn) that adds, for every
// followed record, the integer term of c(w) * x[kin] to y[kout]; the rescale of
// y into the next x.  Every result word is an integer sum, so the result does
// not depend on the grid, the order, the path or the atomics; propagate.h
// states the rule once for the host and the device, abnn_amd/propagate.py
// restates it in numpy.
//
//   k_prop_map      : reads x with 16-B loads (four neurons per lane), ORs eight
//                     lanes' nibbles (x != 0 inside the in-range) into one map
//                     word and writes EVERY word of the map (no memset); adds
//                     the non-zero count and the sum of |x| to header words 4, 5
//                     with one atomic per word and workgroup.
//   k_propagate<kReverse, kSparse, kWide> : workgroups are independent: no
//                     look-back, no ticket, no residency assumption.  Forward,
//                     both the sparse and the dense instance are enqueued; each
//                     reads header word 4 and the one it does not select
//                     returns at once (hops' dead-step idiom: no host round trip).
//       sparse forward: the forward pass of hops.  Streams lo[] and hi[] only
//         (3 B per record), non-temporal, eight records per lane and load, every
//         load of an iteration issued before its first use; tests the src's bit
//         in the map (folded into LDS when few x are non-zero: nearly every
//         record is rejected without a gather), and only for a hit gathers
//         dw[k] and x[src].  Hits are rare: each one is its own add.
//       dense forward, reverse: the stream is scan.h's.  Forward with the src
//         streams; reverse tests the map at dst first and reads lo[k], hi[k]
//         only for a hit.  Runs of equal kout along the wave's consecutive
//         records become one add by the run's head (runs.h).
//       narrow (!kWide, at most kPropNarrowMax out neurons): y is privatised in
//         LDS and flushed once per workgroup with global u64 atomics, zeros
//         skipped.  wide: agent-scope no-return u64 atomics straight into y.
//       The records that no whole sparse load holds (n_syn % 8) are read one at
//       a time by one thread; an odd n_syn's last record inside scan.h's load:
//       nothing is read past record n_syn - 1.
//   k_prop_reduce   : sum |y| and max |y| by one atomic per word and wave.
//   k_prop_rescale  : reads the two words, writes x over the out-range and the
//                     trace row.
#include "propagate.h"
#include "runs.h"
#include "scan.h"

#pragma clang fp contract(off)

namespace abnn {
namespace {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned long long u64;

constexpr uint32_t kNone = kAbsentDst;  // a tombstone's dst, no record
constexpr uint32_t kPropHead = 3;       // header sums per wave: tombstones, followed, skipped
constexpr uint32_t kHead = ABNN_PROP_HEADER_WORDS;

struct PropArgs {
    RecordStream s;
    const int32_t* x;
    const uint32_t* map;
    u64* out;  // header | y
    uint64_t n;
    uint32_t n_nrn, in_first, in_count, out_first, out_m;
    uint32_t flags, path;
    float w_lo, w_hi, base_scale;
};

struct Tally {
    uint32_t tomb, followed, skipped;
};

__global__ __launch_bounds__(kPropPlaneThreads) void k_prop_map(const int32_t* x, uint32_t* map, u64* out, uint32_t n_nrn,
                                                                uint32_t in_first, uint32_t in_count)
{
    __shared__ u64 sums[2 * (kPropPlaneThreads / 64)];
    constexpr uint32_t T = kPropPlaneThreads;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    // one 16-B vector = four neurons per lane, eight lanes = one map word;
    // whole groups of eight lanes, so that every word is written
    const uint32_t n_vec = (uint32_t)((((uint64_t)n_nrn + 31) >> 5) << 3);
    uint32_t nnz = 0;
    uint64_t mag = 0;
    // uniform over the wave: a lane past the end carries an empty nibble through the shuffles
    for (uint32_t base = blockIdx.x * T; base < n_vec; base += gridDim.x * T) {
        const uint32_t v = base + tid;
        const uint64_t at = 4ull * v;
        int32_t e[4] = {0, 0, 0, 0};
        if (at + 4 <= n_nrn) {
            const u32x4 q = *reinterpret_cast<const u32x4*>(x + at);  // x is 16-byte aligned
            e[0] = (int32_t)q.x, e[1] = (int32_t)q.y, e[2] = (int32_t)q.z, e[3] = (int32_t)q.w;
        } else {
            for (uint32_t c = 0; c < 4; ++c)
                if (at + c < n_nrn) e[c] = x[at + c];
        }
        uint32_t nib = 0;
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) {
            const bool in = (uint32_t)(at + c) - in_first < in_count && at + c < n_nrn;
            if (in && e[c] != 0) {
                nib |= 1u << c;
                mag += prop_abs32(e[c]);
            }
        }
        nnz += __popc(nib);
        uint32_t w = nib << (4u * (lane & 7u));
        w |= __shfl_xor(w, 1);
        w |= __shfl_xor(w, 2);
        w |= __shfl_xor(w, 4);
        if ((lane & 7u) == 0 && v < n_vec) map[v >> 3] = w;
    }
    const u64 h[2] = {wave_add((uint64_t)nnz), wave_add(mag)};
    wave_words_to_lds(sums, h, tid);
    if (tid < 2) {
        u64 s = 0;
        for (uint32_t w = 0; w < T / 64; ++w) s += sums[w * 2 + tid];
        if (s) __hip_atomic_fetch_add(out + 4 + tid, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The map word of neuron n, 0 when x[n] cannot count.  The load is issued
// whether or not n is a neuron (n >= N_NRN: the tombstone's src code, a
// tombstone's dst, a record that was never validated -- word 0 then), so that a
// lane's gathers are all issued before the first one is used.  With the fold a
// neuron whose folded bit is clear loads word 0 as well: the lanes of a wave
// that miss share one cache line.
template <bool kFold>
__device__ __forceinline__ uint32_t map_word(const PropArgs& a, const uint32_t* fold, bool use_fold, uint32_t n)
{
    bool may = n < a.n_nrn;
    if (kFold && use_fold) may = may && ((fold[(n >> 5) & (kPropFoldWords - 1u)] >> (n & 31u)) & 1u);
    const uint32_t w = a.map[may ? n >> 5 : 0u];
    return may ? w : 0u;
}

__device__ __forceinline__ bool in_map(const PropArgs& a, uint32_t n, uint32_t word)
{
    return n < a.n_nrn && ((word >> (n & 31u)) & 1u);
}

// The item of one record whose kin is known to lie in the in-range (`cand`:
// and the record is live): the out-range, the weight band, x[kin] != 0, the term.
__device__ __forceinline__ RunItem item(const PropArgs& a, bool cand, uint32_t kin, uint32_t kout, uint32_t wbits, Tally& t)
{
    RunItem it{kRunNone, 0};
    const uint32_t rel = kout - a.out_first;
    const float w = __uint_as_float(wbits);
    if (!cand || rel >= a.out_m || !prop_weight_ok(a.flags, w, a.w_lo, a.w_hi)) return it;
    const int32_t xv = a.x[kin];
    if (xv == 0) return it;
    t.followed += 1;
    int64_t term = 0;
    if (!prop_term(prop_coeff(a.flags, w, a.base_scale), xv, &term)) {
        t.skipped += 1;
        return it;
    }
    it.key = rel;
    it.v = (uint64_t)term;
    return it;
}

template <bool kWide>
__device__ __forceinline__ void emit(const PropArgs& a, u64* lds, uint32_t key, uint64_t v)
{
    if (v == 0) return;
    if (kWide)
        __hip_atomic_fetch_add(a.out + kHead + key, (u64)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
        __hip_atomic_fetch_add(lds + key, (u64)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Sparse forward: `count` (<= 8) records from record `first` on, their src
// codes packed as the streams hold them (lo: 2 B each, hi: 1 B each).
template <bool kWide>
__device__ __forceinline__ void forward_group(const PropArgs& a, const uint32_t* fold, bool use_fold, u64* lds, uint64_t first,
                                              uint32_t count, const uint32_t (&lw)[4], const uint32_t (&hw)[2], Tally& t)
{
    uint32_t src[8], word[8];
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
        src[j] = code_src((lw[j >> 1] >> (16u * (j & 1u))) & 0xFFFFu, (hw[j >> 2] >> (8u * (j & 3u))) & 0xFFu);
        word[j] = map_word<true>(a, fold, use_fold, src[j]);
    }
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
        if (j >= count) continue;
        t.tomb += src[j] == kSrcNone ? 1u : 0u;  // a tombstone's src (abnn.h)
        if (in_map(a, src[j], word[j])) {        // in the in-range, x != 0
            const uint2 r = a.s.dw[first + j];
            const RunItem it = item(a, r.x != kNone, src[j], r.x, r.y, t);
            if (it.key != kRunNone) emit<kWide>(a, lds, it.key, it.v);
        }
    }
}

template <bool kReverse, bool kSparse, bool kWide>
__global__ __launch_bounds__(kPropThreads) void k_propagate(PropArgs a, uint32_t lds_words)
{
    extern __shared__ u64 lds[];  // narrow: y of the out-range; then kPropHead u32 per wave
    __shared__ uint32_t fold[kSparse ? kPropFoldWords : 1];
    constexpr uint32_t T = kPropThreads;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const u64 nnz = __hip_atomic_load(a.out + 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!kReverse) {  // uniform over the grid
        const bool sparse = a.path ? a.path == 1u : nnz * kPropSparseDiv <= a.n_nrn;
        if (sparse != kSparse) return;
    }
    if (!kWide) {
        uint32_t* l32 = reinterpret_cast<uint32_t*>(lds);
        for (uint32_t i = tid; i < lds_words; i += T) l32[i] = 0;
        __syncthreads();
    }

    Tally t{0, 0, 0};
    if (kSparse) {
        // Few non-zero x: the map folded to kPropFoldWords words in LDS (word w ORed
        // into word w mod kPropFoldWords); a record that passes is confirmed
        // against the map.  A map that fits is held whole.  Uniform over the grid.
        const uint32_t bm_words = (uint32_t)(((uint64_t)a.n_nrn + 31) >> 5);
        const bool use_fold = nnz <= kPropFoldMaxNnz || bm_words <= kPropFoldWords;
        if (use_fold) {
            for (uint32_t i = tid; i < kPropFoldWords; i += T) {
                uint32_t w = 0;
                for (uint32_t j = i; j < bm_words; j += kPropFoldWords) w |= a.map[j];
                fold[i] = w;
            }
            __syncthreads();
        }
        constexpr uint32_t U = kPropFwdUnroll;
        const u32x4* lo4 = reinterpret_cast<const u32x4*>(a.s.lo);
        const u32x2* hi2 = reinterpret_cast<const u32x2*>(a.s.hi);
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
                forward_group<kWide>(a, fold, use_fold, lds, 8 * g, g < n_groups ? 8u : 0u, lw, hw, t);
            }
        }
        // the records no whole group holds, one at a time: nothing is read past record n - 1
        const uint32_t rest = (uint32_t)(a.n & 7u);
        if (rest && blockIdx.x == 0 && tid == 0) {
            uint32_t lw[4] = {0, 0, 0, 0}, hw[2] = {0, 0};
            for (uint32_t j = 0; j < rest; ++j) {
                const uint64_t k = 8 * n_groups + j;
                lw[j >> 1] |= (uint32_t)a.s.lo[k] << (16u * (j & 1u));
                hw[j >> 2] |= (uint32_t)a.s.hi[hi_pos(k)] << (8u * (j & 3u));
            }
            forward_group<kWide>(a, fold, use_fold, lds, 8 * n_groups, rest, lw, hw, t);
        }
    } else {
        constexpr uint32_t U = kPropPairUnroll;
        const uint64_t n_pairs = scan_pairs(a.n);
        const uint64_t stride = (uint64_t)gridDim.x * (T * U);
        const auto add = [&](uint32_t key, uint64_t v) { emit<kWide>(a, lds, key, v); };
        // the loop and everything in it is uniform over the wave: a lane past the
        // end carries two absent records through scatter_runs()'s shuffles
        for (uint64_t base = (uint64_t)blockIdx.x * (T * U); base < n_pairs; base += stride) {
            PairLoad<!kReverse, T, U> l;  // an absent record: a dst above N_NRN
            l.load(a.s, base, a.n, tid);
            uint32_t w0[U], w1[U];
            if (kReverse) {
#pragma unroll
                for (uint32_t k = 0; k < U; ++k) {
                    w0[k] = map_word<false>(a, nullptr, false, l.v[k].x);
                    w1[k] = map_word<false>(a, nullptr, false, l.v[k].z);
                }
            }
#pragma unroll
            for (uint32_t k = 0; k < U; ++k) {
                const uint32_t d0 = l.v[k].x, d1 = l.v[k].z;
                t.tomb += (l.valid0(k) && d0 == kNone ? 1u : 0u) + (l.valid1(k) && d1 == kNone ? 1u : 0u);
                RunItem i0, i1;
                if (kReverse) {
                    // a hit (dst in the in-range, x[dst] != 0: the record is live) reads the record's src code
                    const uint64_t p = l.pair(k);
                    const bool h0 = in_map(a, d0, w0[k]), h1 = in_map(a, d1, w1[k]);
                    const uint32_t s0 = h0 ? code_src(a.s.lo[2 * p], a.s.hi[hi_pos(2 * p)]) : kNone;
                    const uint32_t s1 = h1 ? code_src(a.s.lo[2 * p + 1], a.s.hi[hi_pos(2 * p + 1)]) : kNone;
                    i0 = item(a, h0, d0, s0, l.v[k].y, t);
                    i1 = item(a, h1, d1, s1, l.v[k].w, t);
                } else {
                    const uint32_t s0 = l.src0(k), s1 = l.src1(k);
                    i0 = item(a, d0 != kNone && s0 - a.in_first < a.in_count, s0, d0, l.v[k].y, t);
                    i1 = item(a, d1 != kNone && s1 - a.in_first < a.in_count, s1, d1, l.v[k].w, t);
                }
                scatter_runs(lane, i0, i1, add);
            }
        }
    }

    if (!kWide) {
        __syncthreads();
        for (uint32_t j = tid; j < a.out_m; j += T) {
            const u64 s = lds[j];
            if (s) __hip_atomic_fetch_add(a.out + kHead + j, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();  // y's LDS is reused for the waves' header sums
    }

    uint32_t* l32 = reinterpret_cast<uint32_t*>(lds);
    const uint32_t h[kPropHead] = {wave_add(t.tomb), wave_add(t.followed), wave_add(t.skipped)};
    wave_words_to_lds(l32, h, tid);
    if (tid < kPropHead) {
        u64 s = 0;
        for (uint32_t w = 0; w < T / 64; ++w) s += l32[w * kPropHead + tid];
        if (s) __hip_atomic_fetch_add(a.out + 1 + tid, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (blockIdx.x == 0 && tid == 0) a.out[0] = a.n;  // no other thread touches word 0
}

__device__ __forceinline__ uint64_t wave_max64(uint64_t v)
{
    for (int m = 32; m > 0; m >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, m), hi = __shfl_xor((uint32_t)(v >> 32), m);
        const uint64_t o = (uint64_t)hi << 32 | lo;
        v = o > v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(kPropPlaneThreads) void k_prop_reduce(const u64* y, uint32_t m, u64* red)
{
    uint64_t sum = 0, mx = 0;
    for (uint32_t j = blockIdx.x * kPropPlaneThreads + threadIdx.x; j < m; j += gridDim.x * kPropPlaneThreads) {
        const uint64_t v = prop_abs64(y[j]);
        sum += v;
        mx = v > mx ? v : mx;
    }
    sum = wave_add(sum);
    mx = wave_max64(mx);
    if ((threadIdx.x & 63u) == 0 && mx) {  // mx == 0: the wave's y are all zero
        __hip_atomic_fetch_add(red, (u64)sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(red + 1, (u64)mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(kPropPlaneThreads) void k_prop_rescale(const u64* out, uint32_t m, uint32_t out_first, int32_t* x,
                                                                    const u64* red, u64* row)
{
    const u64 mx = red[1];
    const int32_t e = prop_exponent(mx);
    const u64* y = out + kHead;
    for (uint32_t j = blockIdx.x * kPropPlaneThreads + threadIdx.x; j < m; j += gridDim.x * kPropPlaneThreads)
        x[out_first + j] = prop_rescaled(y[j], e);
    if (row && blockIdx.x == 0 && threadIdx.x == 0) {
        row[0] = out[4];
        row[1] = out[5];
        row[2] = red[0];
        row[3] = mx;
        row[4] = (u64)(int64_t)e;
        row[5] = out[2];
        row[6] = out[3];
        row[7] = 0;
    }
}

uint32_t plane_blocks(uint64_t items, uint32_t cus)
{
    const uint64_t b = std::min<uint64_t>(8ull * std::max(1u, cus), (items + kPropPlaneThreads - 1) / kPropPlaneThreads);
    return (uint32_t)std::max<uint64_t>(1, b);
}

template <bool kReverse, bool kSparse>
void launch_instance(const PropArgs& a, bool wide, uint32_t cus, hipStream_t s)
{
    constexpr uint32_t kScratch = (kPropThreads / 64) * kPropHead;  // u32 words for the header sums
    const uint32_t lds_words = wide ? kScratch : std::max(2u * a.out_m, kScratch);
    const uint64_t per_iter = kSparse ? 8ull * kPropThreads * kPropFwdUnroll : 2ull * kPropThreads * kPropPairUnroll;
    // at least one workgroup: sparse, its first thread takes the records that no whole load holds
    const uint32_t grid = std::max(1u, scan_grid(a.n, per_iter, lds_words + (kSparse ? kPropFoldWords : 0u), cus, kScanMaxPerWg));
    const dim3 g(grid), b(kPropThreads);
    if (wide)
        hipLaunchKernelGGL((k_propagate<kReverse, kSparse, true>), g, b, lds_words * 4, s, a, lds_words);
    else
        hipLaunchKernelGGL((k_propagate<kReverse, kSparse, false>), g, b, lds_words * 4, s, a, lds_words);
}

}  // namespace

hipError_t launch_propagate(const SynArrays& syn, uint64_t n, const abnn_propagate_config& cfg, uint64_t n_nrn, float base_scale,
                            const int32_t* x_dev, uint64_t* out_dev, const PropScratch& scratch, uint32_t path,
                            uint32_t cus, hipStream_t s)
{
    const PropRanges r = propagate_ranges(cfg, n_nrn);
    hipError_t e = hipMemsetAsync(out_dev, 0, (ABNN_PROP_HEADER_WORDS + (uint64_t)r.out_count) * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    u64* out = reinterpret_cast<u64*>(out_dev);
    const uint32_t nn = (uint32_t)n_nrn;
    const uint64_t vecs = ((n_nrn + 31) / 32) * 8;
    hipLaunchKernelGGL(k_prop_map, dim3(plane_blocks(vecs, cus)), dim3(kPropPlaneThreads), 0, s, x_dev, scratch.map, out, nn,
                       r.in_first, r.in_count);
    e = hipGetLastError();
    if (e != hipSuccess || n == 0) return e;
    PropArgs a{};
    a.s = record_stream(syn);
    a.x = x_dev;
    a.map = scratch.map;
    a.out = out;
    a.n = n;
    a.n_nrn = nn;
    a.in_first = r.in_first;
    a.in_count = r.in_count;
    a.out_first = r.out_first;
    a.out_m = r.out_count;
    a.flags = cfg.flags;
    a.path = path;
    a.w_lo = cfg.w_lo;
    a.w_hi = cfg.w_hi;
    a.base_scale = base_scale;
    const bool wide = r.out_count > kPropNarrowMax;
    if (cfg.flags & ABNN_PROP_REVERSE) {
        launch_instance<true, false>(a, wide, cus, s);
        return hipGetLastError();
    }
    launch_instance<false, true>(a, wide, cus, s);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    launch_instance<false, false>(a, wide, cus, s);
    return hipGetLastError();
}

hipError_t launch_propagate_rescale(const abnn_propagate_config& cfg, uint64_t n_nrn, const uint64_t* out_dev, int32_t* x_dev,
                                    uint64_t* row_dev, const PropScratch& scratch, uint32_t cus, hipStream_t s)
{
    const PropRanges r = propagate_ranges(cfg, n_nrn);
    hipError_t e = hipMemsetAsync(scratch.red, 0, 2 * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    const u64* out = reinterpret_cast<const u64*>(out_dev);
    u64* red = reinterpret_cast<u64*>(scratch.red);
    const dim3 g(plane_blocks(r.out_count, cus)), b(kPropPlaneThreads);
    hipLaunchKernelGGL(k_prop_reduce, g, b, 0, s, out + kHead, r.out_count, red);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_prop_rescale, g, b, 0, s, out, r.out_count, r.out_first, x_dev, red, reinterpret_cast<u64*>(row_dev));
    return hipGetLastError();
}

}  // namespace abnn
