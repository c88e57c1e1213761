// degree.hip -- the neuron degree census (abnn.h abnn_degree_*):
// one streaming pass over the local records [0, n_syn) that counts, for every
// neuron of a range R, the live records with src == n (fan-out) and with
// dst == n (fan-in) and sums their weights as 2^-24 fixed-point terms.  Every
// result word is an integer sum, so the result does not depend on the grid, the
// order or the atomics; abnn_amd/degree.py restates it in numpy.
//
//   k_degree<kOut, kIn, kWide> : the stream is scan.h's (kDegreeUnroll loads
//       in flight; the kOut instantiations read the two src streams).  Header
//       counts stay in registers and leave with one atomic per word and
//       workgroup.  Workgroups are independent: no look-back, no ticket, no
//       residency assumption.
//     narrow (!kWide, R of at most kDegreeNarrowMax neurons): the planes of R
//       are privatised in LDS (u32 degrees: a workgroup scans at most 2^31
//       records; u64 strengths) and flushed once per workgroup with global u64
//       atomics, zeros skipped.
//     wide (kWide): device-scope no-return u64 atomics straight into the planes.
//
// Aggregation.  A wave's 128 records of one load are consecutive, so keys that
// repeat in consecutive records (the generated graph's dense block: 256 records
// per src; a sorted or a degenerate upload: every record on one neuron) form
// runs along the lanes.  scatter() turns every run into ONE add of the run's
// record count and term sum by the run's first lane, on both paths: the two
// records of a lane merge first; a lane whose records differ hands its first
// record to the lane before it when that lane ends on the same key; then each
// lane holds one item, run heads are found with one ballot, and a wave prefix
// sum gives each head its run's total (last lane's prefix minus its own).  The
// count (at most 192 per wave) rides in the low 8 bits of the 64-bit term sum
// (below 2^39 in magnitude), so one scan serves both.  A wave with no record in
// R skips all of it, and a wave whose items are all different skips the scan.
#include "degree.h"
#include "scan.h"

#pragma clang fp contract(off)

namespace abnn {
namespace {

constexpr uint32_t kNone = kAbsentDst;      // a record outside R, a tombstone, no record
constexpr uint32_t kNoPush = 0xFFFFFFFEu;  // "this lane hands nothing back"

constexpr uint32_t kDegreeHead = 5;  // header sums per wave (wave_words_to_lds packs them at this stride)

struct DegreeArgs {
    RecordStream s;
    unsigned long long* out;
    uint64_t n;
    uint32_t first, m;    // R = [first, first + m)
    uint32_t what;        // the planes of this launch
    uint32_t header;      // this launch writes words 0 / 1 (one launch of a census does)
    uint64_t g_deg[2], g_str[2];  // [out, in]: the planes' word offsets in `out`
    uint32_t l_deg[2], l_str[2];  // narrow: their word offsets in LDS
};

struct Tally {
    uint32_t tomb, n[2], skip[2];
};

// one record's item for one direction: the key (neuron - first, or kNone) and
// the packed {term sum << 8 | record count}
struct Item {
    uint32_t key;
    uint64_t v;
};

template <bool kWide, int D>
__device__ __forceinline__ void emit(const DegreeArgs& a, uint32_t* lds, uint32_t key, uint64_t v)
{
    const uint32_t c = (uint32_t)(v & 0xFFu);
    const unsigned long long s = (unsigned long long)((long long)v >> 8);
    const bool deg = a.what & (D ? ABNN_DEG_IN : ABNN_DEG_OUT);
    const bool str = (a.what & (D ? ABNN_DEG_IN_W : ABNN_DEG_OUT_W)) && s != 0;
    if (kWide) {
        if (deg) __hip_atomic_fetch_add(a.out + a.g_deg[D] + key, (unsigned long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (str) __hip_atomic_fetch_add(a.out + a.g_str[D] + key, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        if (deg) __hip_atomic_fetch_add(lds + a.l_deg[D] + key, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (str)
            __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(lds + a.l_str[D]) + key, s, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

// Cross-lane moves on the VALU (DPP), every lane of the wave active: a lane
// with no source lane gets 0.  Controls: row_shr:n = 0x110 + n (lane l of a
// 16-lane row reads lane l - n), wave_shl:1 / wave_shr:1 (lane l reads lane
// l + 1 / l - 1 of the wave), row_bcast:15 / :31 (lane 15 / 31 to the whole
// next row / the upper half; the row mask names the rows that receive).
constexpr int kDppWaveShl1 = 0x130, kDppWaveShr1 = 0x138, kDppBcast15 = 0x142, kDppBcast31 = 0x143;

template <int kCtrl, int kRows = 0xF>
__device__ __forceinline__ uint32_t dpp(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kCtrl, kRows, 0xF, false);
}

template <int kCtrl, int kRows = 0xF>
__device__ __forceinline__ uint64_t dpp(uint64_t v)
{
    return (uint64_t)dpp<kCtrl, kRows>((uint32_t)v) | (uint64_t)dpp<kCtrl, kRows>((uint32_t)(v >> 32)) << 32;
}

// inclusive prefix sum over the wave's 64 lanes, modulo 2^64
__device__ __forceinline__ uint64_t wave_prefix(uint64_t v)
{
    // a lane without a source lane (the row's first n, the rows outside the mask) adds the 0 it got
    v += dpp<0x111>(v);
    v += dpp<0x112>(v);
    v += dpp<0x114>(v);
    v += dpp<0x118>(v);
    v += dpp<kDppBcast15, 0xA>(v);
    v += dpp<kDppBcast31, 0xC>(v);
    return v;
}

// The wave's items of one load (lane l holds records 2l and 2l + 1 of 128
// consecutive ones) for direction D.  Every lane of the wave calls it.
template <bool kWide, int D>
__device__ __forceinline__ void scatter(const DegreeArgs& a, uint32_t* lds, uint32_t lane, Item r0, Item r1)
{
    if (!__any(r0.key != kNone || r1.key != kNone)) return;
    const bool uni = r0.key == r1.key;
    uint64_t tv = uni ? r0.v + r1.v : r1.v;  // the lane's item has key r1.key
    // lane 0's prev_tail and lane 63's next_* are not used
    const uint32_t prev_tail = dpp<kDppWaveShr1>(r1.key);
    const uint32_t next_head = dpp<kDppWaveShl1>(uni ? kNoPush : r0.key);
    const uint64_t next_v = dpp<kDppWaveShl1>(r0.v);
    if (lane < 63 && next_head == r1.key && r1.key != kNone) tv += next_v;
    const bool handed = !uni && lane > 0 && prev_tail == r0.key;
    if (!uni && !handed && r0.key != kNone) emit<kWide, D>(a, lds, r0.key, r0.v);
    const bool head = lane == 0 || !uni || prev_tail != r1.key;
    const uint64_t heads = __ballot(head);
    if (heads == ~0ull) {
        if (r1.key != kNone) emit<kWide, D>(a, lds, r1.key, tv);
        return;
    }
    const uint64_t p = wave_prefix(tv);
    if (heads == 1ull) {  // the wave is one run: its total is the last lane's prefix
        const uint64_t total = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)p, 63) |
                               (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(p >> 32), 63) << 32;
        if (lane == 0 && r1.key != kNone) emit<kWide, D>(a, lds, r1.key, total);
        return;
    }
    const uint64_t above = lane == 63 ? 0ull : heads & (~0ull << (lane + 1));
    const uint32_t last = above ? (uint32_t)__ffsll((unsigned long long)above) - 2u : 63u;  // the run's last lane
    const uint64_t pe = __shfl((unsigned long long)p, (int)last);
    if (head && r1.key != kNone) emit<kWide, D>(a, lds, r1.key, pe - p + tv);
}

// One record's items; counts the header words into t.
template <bool kOut, bool kIn>
__device__ __forceinline__ void items(const DegreeArgs& a, bool valid, uint32_t src, uint32_t dst, uint32_t wbits, Tally& t,
                                      Item& o, Item& i)
{
    const bool tomb = dst == kNone;
    t.tomb += (valid && tomb) ? 1u : 0u;
    const bool live = valid && !tomb;
    const float w = __uint_as_float(wbits);
    const bool summable = fabsf(w) < 128.0f;  // false for NaN and +-inf
    const int32_t q = summable ? (int32_t)(w * 16777216.0f) : 0;
    const uint64_t v = (uint64_t)((int64_t)q * 256) + 1u;
    o = Item{kNone, 0};
    i = Item{kNone, 0};
    if (kOut) {
        const uint32_t rel = src - a.first;
        if (live && rel < a.m) {
            o = Item{rel, v};
            t.n[0] += 1;
            t.skip[0] += summable ? 0u : 1u;
        }
    }
    if (kIn) {
        const uint32_t rel = dst - a.first;
        if (live && rel < a.m) {
            i = Item{rel, v};
            t.n[1] += 1;
            t.skip[1] += summable ? 0u : 1u;
        }
    }
}

template <bool kOut, bool kIn, bool kWide>
__global__ __launch_bounds__(kDegreeThreads) void k_degree(DegreeArgs a, uint32_t lds_words)
{
    extern __shared__ uint32_t lds[];  // narrow: the planes of R; then kDegreeHead words per wave
    constexpr uint32_t T = kDegreeThreads, U = kDegreeUnroll;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    if (!kWide) {
        for (uint32_t i = tid; i < lds_words; i += T) lds[i] = 0;
        __syncthreads();
    }

    Tally t{0, {0, 0}, {0, 0}};
    const uint64_t n_pairs = scan_pairs(a.n);
    const uint64_t stride = (uint64_t)gridDim.x * (T * U);
    // the loop and everything in it is uniform over the wave: a lane past the
    // end carries two absent records through scatter()'s shuffles
    for (uint64_t base = (uint64_t)blockIdx.x * (T * U); base < n_pairs; base += stride) {
        PairLoad<kOut, T, U> l;
        l.load(a.s, base, a.n, tid);
#pragma unroll
        for (uint32_t k = 0; k < U; ++k) {
            Item o0, i0, o1, i1;
            items<kOut, kIn>(a, l.valid0(k), l.src0(k), l.v[k].x, l.v[k].y, t, o0, i0);
            items<kOut, kIn>(a, l.valid1(k), l.src1(k), l.v[k].z, l.v[k].w, t, o1, i1);
            if (kOut) scatter<kWide, 0>(a, lds, lane, o0, o1);
            if (kIn) scatter<kWide, 1>(a, lds, lane, i0, i1);
        }
    }

    if (!kWide) {
        __syncthreads();
        for (uint32_t j = tid; j < a.m; j += T) {
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                if (a.what & (d ? ABNN_DEG_IN : ABNN_DEG_OUT)) {
                    const uint32_t c = lds[a.l_deg[d] + j];
                    if (c) atomicAdd(a.out + a.g_deg[d] + j, (unsigned long long)c);
                }
                if (a.what & (d ? ABNN_DEG_IN_W : ABNN_DEG_OUT_W)) {
                    const unsigned long long s = reinterpret_cast<const unsigned long long*>(lds + a.l_str[d])[j];
                    if (s) atomicAdd(a.out + a.g_str[d] + j, s);
                }
            }
        }
        __syncthreads();  // the planes' LDS is reused for the waves' header sums
    }

    // words 1..5; a strength plane that is not asked leaves its skipped word 0
    const uint32_t h[kDegreeHead] = {wave_add(a.header ? t.tomb : 0u), wave_add(t.n[0]), wave_add(t.n[1]),
                                     wave_add((a.what & ABNN_DEG_OUT_W) ? t.skip[0] : 0u),
                                     wave_add((a.what & ABNN_DEG_IN_W) ? t.skip[1] : 0u)};
    wave_words_to_lds(lds, h, tid);
    if (tid < kDegreeHead) {
        unsigned long long s = 0;
        for (uint32_t w = 0; w < T / 64; ++w) s += lds[w * kDegreeHead + tid];
        if (s) atomicAdd(a.out + 1 + tid, s);
    }
    if (a.header && blockIdx.x == 0 && tid == 0) a.out[0] = a.n;  // no other thread touches word 0
}

// LDS bytes of a narrow launch's planes
uint32_t plane_bytes(uint32_t what, uint32_t m)
{
    uint32_t b = 0;
    if (what & ABNN_DEG_OUT_W) b += 8 * m;
    if (what & ABNN_DEG_IN_W) b += 8 * m;
    if (what & ABNN_DEG_OUT) b += 4 * m;
    if (what & ABNN_DEG_IN) b += 4 * m;
    return b;
}

hipError_t launch_one(DegreeArgs a, bool wide, uint32_t cus, hipStream_t s)
{
    constexpr uint32_t kScratch = (kDegreeThreads / 64) * kDegreeHead;  // words for the header sums
    uint32_t lds_words = kScratch;
    if (!wide) {
        // 64-bit strengths first (8-byte aligned), then the u32 degrees
        uint32_t off = 0;
        if (a.what & ABNN_DEG_OUT_W) a.l_str[0] = off, off += 2 * a.m;
        if (a.what & ABNN_DEG_IN_W) a.l_str[1] = off, off += 2 * a.m;
        if (a.what & ABNN_DEG_OUT) a.l_deg[0] = off, off += a.m;
        if (a.what & ABNN_DEG_IN) a.l_deg[1] = off, off += a.m;
        lds_words = std::max(off, kScratch);
    }
    const uint32_t grid = scan_grid(a.n, 2ull * kDegreeThreads * kDegreeUnroll, lds_words, cus, kScanMaxPerWg);
    const bool o = a.what & (ABNN_DEG_OUT | ABNN_DEG_OUT_W), i = a.what & (ABNN_DEG_IN | ABNN_DEG_IN_W);
    const dim3 g(grid), b(kDegreeThreads);
    const uint32_t bytes = lds_words * 4;
#define ABNN_DEGREE_LAUNCH(O, I)                                                               \
    do {                                                                                       \
        if (wide)                                                                              \
            hipLaunchKernelGGL((k_degree<O, I, true>), g, b, bytes, s, a, lds_words);          \
        else                                                                                   \
            hipLaunchKernelGGL((k_degree<O, I, false>), g, b, bytes, s, a, lds_words);         \
    } while (0)
    if (o && i)
        ABNN_DEGREE_LAUNCH(true, true);
    else if (o)
        ABNN_DEGREE_LAUNCH(true, false);
    else
        ABNN_DEGREE_LAUNCH(false, true);
#undef ABNN_DEGREE_LAUNCH
    return hipGetLastError();
}

}  // namespace

hipError_t launch_degree(const SynArrays& syn, uint64_t n, const abnn_degree_config& cfg, uint64_t n_nrn,
                         uint64_t* out_dev, uint32_t cus, hipStream_t s)
{
    const uint64_t m = cfg.count ? (uint64_t)cfg.count : n_nrn;
    const uint64_t words = ABNN_DEGREE_HEADER_WORDS + (uint64_t)__builtin_popcount(cfg.what) * m;
    hipError_t e = hipMemsetAsync(out_dev, 0, words * sizeof(uint64_t), s);
    if (e != hipSuccess || n == 0) return e;
    DegreeArgs a{};
    a.s = record_stream(syn);
    a.out = reinterpret_cast<unsigned long long*>(out_dev);
    a.n = n;
    a.first = cfg.count ? cfg.first : 0u;
    a.m = (uint32_t)m;
    // the planes follow the header in increasing bit order
    uint64_t off = ABNN_DEGREE_HEADER_WORDS;
    if (cfg.what & ABNN_DEG_OUT) a.g_deg[0] = off, off += m;
    if (cfg.what & ABNN_DEG_IN) a.g_deg[1] = off, off += m;
    if (cfg.what & ABNN_DEG_OUT_W) a.g_str[0] = off, off += m;
    if (cfg.what & ABNN_DEG_IN_W) a.g_str[1] = off, off += m;
    const bool wide = m > kDegreeNarrowMax;
    a.what = cfg.what;
    a.header = 1;
    if (wide || plane_bytes(cfg.what, a.m) <= kDegreeLdsBytes) return launch_one(a, wide, cus, s);
    // the four planes of a long narrow range: one scan per direction
    a.what = cfg.what & (ABNN_DEG_OUT | ABNN_DEG_OUT_W);
    e = launch_one(a, false, cus, s);
    if (e != hipSuccess) return e;
    a.what = cfg.what & (ABNN_DEG_IN | ABNN_DEG_IN_W);
    a.header = 0;
    return launch_one(a, false, cus, s);
}

}  // namespace abnn
