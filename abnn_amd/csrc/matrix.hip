// matrix.hip -- the population connectivity matrix (abnn.h abnn_matrix_*,
// DESIGN.md §9): one streaming pass over the local records [0, n_syn) that
// counts, for every pair (a, b) of P populations, the live records from a to b
// and sums their weights (and their fire probabilities) as 2^-24 fixed-point
// terms.  Every result word is an integer sum, so the result does not depend on
// the grid, the order or the atomics; abnn_amd/matrix.py restates it in numpy.
//
//   k_matrix_head : words 0, 9, 10 and, for BOUNDS, word 11 and the sizes.
//   k_matrix_pack : LABELS.  Counts the sizes with per-workgroup LDS counters
//       and (packed path) turns the u32 label plane into the handle's u8 plane,
//       0xFF = none, so that the scan's two gathers per record touch N_NRN bytes.
//   k_matrix<kLabels, kRuns> : the stream is scan.h's PairLoad<true, ...>
//       (kMatUnroll loads in flight, the two src streams: 11 B per record).  The
//       P x P cells of every plane asked are privatised in LDS (u32 counts: a
//       workgroup scans fewer than 2^31 records; u64 sums) and flushed once per
//       workgroup with global u64 atomics, zeros skipped.  Header counts stay in
//       registers and leave with one atomic per word and workgroup.  Both sum
//       planes of many populations exceed 64 KiB and take two scans
//       (launch_matrix).  Workgroups
//       are independent: no look-back, no ticket, no residency assumption.
//
// Contention.  In the generated graph nearly every record is hidden -> hidden:
// with the built-in populations almost every record hits ONE cell.  kRuns sends
// a wave's 128 consecutive records of one load through runs.h scatter_runs: its
// ballot of run heads finds the wave whose lanes all hold one cell (heads == 1),
// reduces the packed {term sum << 8 | count} along the wave and lets lane 0 add
// once; a mixed wave adds once per run of equal cells.  !kRuns is the baseline
// the bench compares with: one LDS atomic per record and plane.
//
// BOUNDS lookup.  The P - 1 inner bounds sit in LDS, padded with 0xFFFFFFFF to
// 63 entries; pop(n) is the number of inner bounds <= n, found by a branch-free
// binary search of ceil(log2 P) <= 6 steps, valid when bounds[0] <= n <
// bounds[P].  No memory gathers.
#include "matrix.h"
#include "runs.h"
#include "scan.h"

#pragma clang fp contract(off)

namespace abnn {
namespace {

constexpr uint32_t kMatHead = 8;        // header sums per wave: words 1..8
constexpr uint32_t kMatBoundsLds = 64;  // the inner bounds' LDS words (63 used)
constexpr uint32_t kPackNone = 0xFFu;

struct MatArgs {
    RecordStream s;
    unsigned long long* out;
    uint64_t n;
    uint32_t n_nrn, pops, what, flags;
    uint32_t header;  // this launch writes words 1..6 (one launch of a matrix does)
    float w_lo, w_hi, base_scale;
    const uint8_t* pack;     // LABELS, packed path (null: the direct path)
    const uint32_t* labels;  // LABELS
    uint64_t g_cnt, g_w, g_p;  // the planes' word offsets in `out`
    uint32_t l_cnt, l_w, l_p;  // their word offsets in LDS
    uint32_t l_bounds, l_head, lds_clear;
    uint32_t top;  // the binary search's first step: 2^(ceil(log2 P) - 1), 0 for P == 1
    uint32_t bounds[ABNN_MATRIX_MAX_POPS + 1];
};

struct MatHeadArgs {
    unsigned long long* out;
    uint64_t n;
    uint32_t n_nrn, pops, labels;
    uint32_t bounds[ABNN_MATRIX_MAX_POPS + 1];
};

__global__ __launch_bounds__(64) void k_matrix_head(MatHeadArgs a)
{
    const uint32_t tid = threadIdx.x;
    if (tid == 0) {
        a.out[0] = a.n;
        a.out[9] = a.pops;
        a.out[10] = a.n_nrn;
        if (!a.labels) a.out[11] = a.bounds[a.pops] - a.bounds[0];
    }
    if (!a.labels && tid < a.pops) a.out[kMatSizesAt + tid] = a.bounds[tid + 1] - a.bounds[tid];
}

// Four neurons per thread: the sizes, and with `pack` one u32 of four packed bytes.
__global__ __launch_bounds__(kMatPlaneThreads) void k_matrix_pack(const uint32_t* labels, uint32_t n_nrn, uint32_t pops,
                                                                  uint8_t* pack, unsigned long long* out)
{
    __shared__ uint32_t cnt[ABNN_MATRIX_MAX_POPS];
    const uint32_t tid = threadIdx.x;
    if (tid < ABNN_MATRIX_MAX_POPS) cnt[tid] = 0;
    __syncthreads();
    const uint64_t quads = ((uint64_t)n_nrn + 3) / 4;
    for (uint64_t q = (uint64_t)blockIdx.x * kMatPlaneThreads + tid; q < quads; q += (uint64_t)gridDim.x * kMatPlaneThreads) {
        const uint64_t n0 = 4 * q;
        uint32_t word = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            uint32_t v = kPackNone;
            if (n0 + j < n_nrn) {
                const uint32_t l = labels[n0 + j];
                if (l < pops) {
                    v = l;
                    __hip_atomic_fetch_add(&cnt[l], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
            word |= v << (8 * j);
        }
        if (pack) {
            if (n0 + 3 < n_nrn) {
                reinterpret_cast<uint32_t*>(pack)[q] = word;  // the plane is hipMalloc-aligned
            } else {
                for (uint32_t j = 0; n0 + j < n_nrn; ++j) pack[n0 + j] = (uint8_t)(word >> (8 * j));
            }
        }
    }
    __syncthreads();
    if (tid < pops) {
        const uint32_t c = cnt[tid];
        if (c) {
            atomicAdd(out + kMatSizesAt + tid, (unsigned long long)c);
            atomicAdd(out + 11, (unsigned long long)c);
        }
    }
}

struct Tally {
    uint32_t tomb, counted, src_un, dst_un, both_un, oob, skip_w, skip_p;
};

// one record, classified: its cell (kRunNone when it is not counted) and its two terms
struct Rec {
    uint32_t cell;
    int32_t qw, qp;
};

__device__ __forceinline__ uint32_t pop_bounds(const MatArgs& a, const uint32_t* lb, uint32_t n)
{
    uint32_t pos = 0;
    for (uint32_t s = a.top; s; s >>= 1) pos += lb[pos + s - 1] <= n ? s : 0u;  // pos + s - 1 <= 62
    return (n >= a.bounds[0] && n < a.bounds[a.pops]) ? pos : kMatNone;
}

__device__ __forceinline__ uint32_t pop_labels(const MatArgs& a, bool use, uint32_t n)
{
    if (!use || n >= a.n_nrn) return kMatNone;  // an id that is no neuron is never an index
    if (a.pack) {
        const uint32_t v = a.pack[n];
        return v == kPackNone ? kMatNone : v;
    }
    const uint32_t v = a.labels[n];
    return v < a.pops ? v : kMatNone;
}

template <bool kLabels>
__device__ __forceinline__ Rec classify(const MatArgs& a, const uint32_t* lb, bool valid, uint32_t src, uint32_t dst,
                                        uint32_t wbits, Tally& t)
{
    const bool tomb = dst == kAbsentDst;
    t.tomb += (valid && tomb) ? 1u : 0u;
    const bool live = valid && !tomb;
    const float w = __uint_as_float(wbits);
    const bool band = mat_weight_ok(a.flags, w, a.w_lo, a.w_hi);
    t.oob += (live && !band) ? 1u : 0u;
    const bool use = live && band;
    uint32_t pa, pb;
    if (kLabels) {
        pa = pop_labels(a, use, src);
        pb = pop_labels(a, use, dst);
    } else {
        pa = pop_bounds(a, lb, src);
        pb = pop_bounds(a, lb, dst);
    }
    const bool sa = pa != kMatNone, sb = pb != kMatNone;
    const bool counted = use && sa && sb;
    t.counted += counted ? 1u : 0u;
    t.src_un += (use && !sa && sb) ? 1u : 0u;
    t.dst_un += (use && sa && !sb) ? 1u : 0u;
    t.both_un += (use && !sa && !sb) ? 1u : 0u;
    Rec r{kRunNone, 0, 0};
    if (counted) {
        r.cell = pa * a.pops + pb;
        if (a.what & ABNN_MAT_W) t.skip_w += mat_term(w, &r.qw) ? 0u : 1u;
        if (a.what & ABNN_MAT_P) t.skip_p += mat_term(mat_fire_p(w, a.base_scale), &r.qp) ? 0u : 1u;
    }
    return r;
}

// v = {term sum << 8 | record count}: the count to the COUNT plane (when this
// value carries it), the sum to the u64 plane at LDS word l_sum
__device__ __forceinline__ void add_cell(uint32_t* lds, uint32_t l_cnt, uint32_t l_sum, uint32_t cell, uint64_t v)
{
    const uint32_t c = (uint32_t)(v & 0xFFu);
    const unsigned long long s = (unsigned long long)((long long)v >> 8);
    if (c) __hip_atomic_fetch_add(lds + l_cnt + cell, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (s)
        __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(lds + l_sum) + cell, s, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
}

// One scatter takes one load of one wave: two records per lane, so a run's
// count is at most kScatterRecords and fits the packed value's low 8 bits, and
// its term sum (|q| < 2^31 each) stays far below 2^55.  A record that is not
// counted (cell kRunNone) carries its count bit all the same: lanes without a
// cell form runs of their own that scatter_runs never emits.
constexpr uint32_t kScatterRecords = 2 * 64;
static_assert(kScatterRecords <= 255, "the packed count is 8 bits: a scatter may not take more records");
__device__ __forceinline__ uint64_t packed(int32_t q, uint64_t count) { return (uint64_t)((int64_t)q * 256) + count; }

// the two records of a lane for one plane; every lane of the wave calls it
template <bool kRuns>
__device__ __forceinline__ void scatter(uint32_t* lds, uint32_t l_cnt, uint32_t l_sum, uint32_t lane, uint32_t cell0,
                                        uint64_t v0, uint32_t cell1, uint64_t v1)
{
    if (kRuns) {
        scatter_runs(lane, RunItem{cell0, v0}, RunItem{cell1, v1},
                     [&](uint32_t cell, uint64_t v) { add_cell(lds, l_cnt, l_sum, cell, v); });
    } else {
        if (cell0 != kRunNone) add_cell(lds, l_cnt, l_sum, cell0, v0);
        if (cell1 != kRunNone) add_cell(lds, l_cnt, l_sum, cell1, v1);
    }
}

template <bool kLabels, bool kRuns>
__global__ __launch_bounds__(kMatThreads) void k_matrix(MatArgs a)
{
    extern __shared__ unsigned long long lds64[];  // the u64 sums, the u32 counts, the inner bounds, the waves' header sums
    uint32_t* lds = reinterpret_cast<uint32_t*>(lds64);
    constexpr uint32_t T = kMatThreads, U = kMatUnroll;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (uint32_t i = tid; i < a.lds_clear; i += T) lds[i] = 0;
    uint32_t* lb = lds + a.l_bounds;
    if (tid < kMatBoundsLds) lb[tid] = (tid + 1 < a.pops) ? a.bounds[tid + 1] : 0xFFFFFFFFu;
    __syncthreads();

    Tally t{0, 0, 0, 0, 0, 0, 0, 0};
    const uint64_t n_pairs = scan_pairs(a.n);
    const uint64_t stride = (uint64_t)gridDim.x * (T * U);
    // the loop and everything in it is uniform over the wave: a lane past the
    // end carries two absent records through scatter_runs' shuffles
    for (uint64_t base = (uint64_t)blockIdx.x * (T * U); base < n_pairs; base += stride) {
        PairLoad<true, T, U> l;
        l.load(a.s, base, a.n, tid);
#pragma unroll
        for (uint32_t k = 0; k < U; ++k) {
            const Rec r0 = classify<kLabels>(a, lb, l.valid0(k), l.src0(k), l.v[k].x, l.v[k].y, t);
            const Rec r1 = classify<kLabels>(a, lb, l.valid1(k), l.src1(k), l.v[k].z, l.v[k].w, t);
            uint64_t c1 = (a.what & ABNN_MAT_COUNT) ? 1u : 0u;  // the first plane's value carries the count
            if (a.what & ABNN_MAT_W) {
                scatter<kRuns>(lds, a.l_cnt, a.l_w, lane, r0.cell, packed(r0.qw, c1), r1.cell, packed(r1.qw, c1));
                c1 = 0;
            }
            if (a.what & ABNN_MAT_P) {
                scatter<kRuns>(lds, a.l_cnt, a.l_p, lane, r0.cell, packed(r0.qp, c1), r1.cell, packed(r1.qp, c1));
                c1 = 0;
            }
            if (c1) scatter<kRuns>(lds, a.l_cnt, 0, lane, r0.cell, 1u, r1.cell, 1u);  // COUNT alone: no sum
        }
    }

    __syncthreads();
    const uint32_t cells = a.pops * a.pops;
    for (uint32_t j = tid; j < cells; j += T) {
        if (a.what & ABNN_MAT_COUNT) {
            const uint32_t c = lds[a.l_cnt + j];
            if (c) atomicAdd(a.out + a.g_cnt + j, (unsigned long long)c);
        }
        if (a.what & ABNN_MAT_W) {
            const unsigned long long s = reinterpret_cast<const unsigned long long*>(lds + a.l_w)[j];
            if (s) atomicAdd(a.out + a.g_w + j, s);
        }
        if (a.what & ABNN_MAT_P) {
            const unsigned long long s = reinterpret_cast<const unsigned long long*>(lds + a.l_p)[j];
            if (s) atomicAdd(a.out + a.g_p + j, s);
        }
    }

    // words 1..8; a sum plane that is not asked leaves its word 0
    const uint32_t hd = a.header;
    const uint32_t h[kMatHead] = {wave_add(hd ? t.tomb : 0u),    wave_add(hd ? t.counted : 0u), wave_add(hd ? t.src_un : 0u),
                                  wave_add(hd ? t.dst_un : 0u),  wave_add(hd ? t.both_un : 0u), wave_add(hd ? t.oob : 0u),
                                  wave_add(t.skip_w),            wave_add(t.skip_p)};
    wave_words_to_lds(lds + a.l_head, h, tid);
    if (tid < kMatHead) {
        unsigned long long s = 0;
        for (uint32_t w = 0; w < T / 64; ++w) s += lds[a.l_head + w * kMatHead + tid];
        if (s) atomicAdd(a.out + 1 + tid, s);
    }
}

// LDS bytes of a launch's accumulators, bounds and header sums
uint32_t lds_bytes(uint32_t what, uint32_t pops)
{
    const uint32_t cells = pops * pops;
    uint32_t b = (kMatBoundsLds + (kMatThreads / 64) * kMatHead) * 4;
    if (what & ABNN_MAT_COUNT) b += 4 * cells;
    if (what & ABNN_MAT_W) b += 8 * cells;
    if (what & ABNN_MAT_P) b += 8 * cells;
    return b;
}

hipError_t launch_one(MatArgs a, bool labels, bool runs, uint32_t cus, hipStream_t s)
{
    const uint32_t cells = a.pops * a.pops;
    // the 64-bit sums first (8-byte aligned), then the u32 counts, the bounds, the header sums
    uint32_t off = 0;
    if (a.what & ABNN_MAT_W) a.l_w = off, off += 2 * cells;
    if (a.what & ABNN_MAT_P) a.l_p = off, off += 2 * cells;
    a.l_cnt = off;
    if (a.what & ABNN_MAT_COUNT) off += cells;
    a.lds_clear = off;
    a.l_bounds = off, off += kMatBoundsLds;
    a.l_head = off, off += (kMatThreads / 64) * kMatHead;
    const uint32_t lds_words = off;
    const uint32_t grid = scan_grid(a.n, 2ull * kMatThreads * kMatUnroll, lds_words, cus, kScanMaxPerWg);
    const dim3 g(grid), b(kMatThreads);
    const uint32_t bytes = lds_words * 4;
    if (labels && runs)
        hipLaunchKernelGGL((k_matrix<true, true>), g, b, bytes, s, a);
    else if (labels)
        hipLaunchKernelGGL((k_matrix<true, false>), g, b, bytes, s, a);
    else if (runs)
        hipLaunchKernelGGL((k_matrix<false, true>), g, b, bytes, s, a);
    else
        hipLaunchKernelGGL((k_matrix<false, false>), g, b, bytes, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_matrix(const SynArrays& syn, uint64_t n, const abnn_matrix_config& cfg, const uint32_t* bounds,
                         const uint32_t* labels_dev, uint64_t n_nrn, float base_scale, uint8_t* pack_dev, uint32_t path,
                         uint64_t* out_dev, uint32_t cus, hipStream_t s)
{
    const bool labels = cfg.flags & ABNN_MAT_LABELS;
    const bool runs = path == kMatPathAuto || path == kMatPathRunsPacked || path == kMatPathRunsDirect;
    const bool direct = path == kMatPathRunsDirect || path == kMatPathAtomicDirect;
    const uint32_t P = cfg.pops;
    const uint64_t cells = (uint64_t)P * P;
    unsigned long long* out = reinterpret_cast<unsigned long long*>(out_dev);
    hipError_t e = hipMemsetAsync(out_dev, 0, matrix_words(&cfg) * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;

    MatHeadArgs h{};
    h.out = out;
    h.n = n;
    h.n_nrn = (uint32_t)n_nrn;
    h.pops = P;
    h.labels = labels ? 1u : 0u;
    if (!labels)
        for (uint32_t j = 0; j <= P; ++j) h.bounds[j] = bounds[j];
    hipLaunchKernelGGL(k_matrix_head, dim3(1), dim3(64), 0, s, h);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (labels) {
        const uint64_t quads = (n_nrn + 3) / 4;
        const uint32_t grid = (uint32_t)std::min<uint64_t>((quads + kMatPlaneThreads - 1) / kMatPlaneThreads,
                                                           (uint64_t)std::max(1u, cus) * 8);
        hipLaunchKernelGGL(k_matrix_pack, dim3(grid), dim3(kMatPlaneThreads), 0, s, labels_dev, (uint32_t)n_nrn, P,
                           direct ? nullptr : pack_dev, out);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (n == 0) return hipSuccess;

    MatArgs a{};
    a.s = record_stream(syn);
    a.out = out;
    a.n = n;
    a.n_nrn = (uint32_t)n_nrn;
    a.pops = P;
    a.flags = cfg.flags;
    a.w_lo = cfg.w_lo;
    a.w_hi = cfg.w_hi;
    a.base_scale = base_scale;
    a.pack = (labels && !direct) ? pack_dev : nullptr;
    a.labels = labels_dev;
    a.top = 0;
    while (P > 1 && (a.top ? 2 * a.top : 1u) < P) a.top = a.top ? 2 * a.top : 1u;  // 2^(ceil(log2 P) - 1)
    if (!labels)
        for (uint32_t j = 0; j <= P; ++j) a.bounds[j] = bounds[j];
    // the planes follow the sizes in increasing bit order
    uint64_t off = kMatSizesAt + P;
    if (cfg.what & ABNN_MAT_COUNT) a.g_cnt = off, off += cells;
    if (cfg.what & ABNN_MAT_W) a.g_w = off, off += cells;
    if (cfg.what & ABNN_MAT_P) a.g_p = off, off += cells;
    a.what = cfg.what;
    a.header = 1;
    if (lds_bytes(cfg.what, P) <= kMatLdsBytes) return launch_one(a, labels, runs, cus, s);
    // Both sum planes of many populations (W | P of 64, COUNT | W | P of more than 57) do not fit one
    // workgroup's LDS: two scans, the planes asked without P (with the header), then P alone.  Each fits:
    // COUNT | W of 64 populations is 48.5 KiB.
    a.what = cfg.what & ~ABNN_MAT_P;
    if ((e = launch_one(a, labels, runs, cus, s)) != hipSuccess) return e;
    a.what = ABNN_MAT_P;
    a.header = 0;
    return launch_one(a, labels, runs, cus, s);
}

}  // namespace abnn
