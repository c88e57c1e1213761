// components.hip -- connected components (abnn.h abnn_components_*, DESIGN.md
// §9): the weakly connected components of the local records [0, n_syn) over a
// neuron range R, one streaming pass over the records with a lock-free
// union-find in a one-u32-per-neuron label plane.  The result is canonical
// (every neuron's label is the smallest neuron id of its component), so it
// depends on neither the grid nor the order nor the timing;
// abnn_amd/components.py restates it in numpy.
//
// The plane.  Invariant: plane[x] <= x, and plane[x] is an ancestor-or-self of
// x in x's tree.  find(x) follows plane[] to its fixed point; every step
// strictly decreases the id, so it ends after at most x - first steps.
//   unite(u, v): loop { ru = find(u); rv = find(v); if ru == rv done;
//                       make ru > rv; old = CAS(&plane[ru], ru, rv);
//                       if old == ru done; else u = old }
// The hook is an agent-scope relaxed compare-and-swap whose returned value is
// used: the final partition and its smallest-id labels do not depend on which
// hook wins.  Every other write to the plane inside LINK, MERGE and FLATTEN is
// a no-return agent-scope atomicMin (the path shortcut plane[x] = min(plane[x],
// grandparent), the flatten's write): no plain store touches the plane while
// another workgroup may read it.  The plane therefore only decreases, and a
// stale read (this CU's L1, another XCD's L2) is an OLDER ANCESTOR: it is still
// an ancestor, so a walk from it still ends at the tree's root; a stale "root"
// costs a failed CAS, whose returned value is fresh and strictly smaller, so
// the retry loop is bounded as well.  A root that a stale read takes for the
// hook's target (rv) may no longer be a root: hooking under any smaller node of
// another tree keeps the invariant.  The root of a converged component is its
// smallest id -- it can never get a smaller parent inside its own component --
// which is why the labels are canonical.  Workgroups never wait for one
// another: no look-back, no ticket, no residency assumption.  Both loops carry
// a hard cap as well (count steps, 2 x count retries: the bounds above); a lane
// that reaches it puts a code into word 7 with an atomic and stops.
//
//   k_comp_begin   : words 0..39 zero, plane[n] = n on R and NONE elsewhere.
//   k_comp_link<kWeight, kSettled> : records [k0, k1) as scan.h's PairLoad
//                    <kSrc = true> takes them (16-B {dst, w} pairs plus lo /
//                    hi, non-temporal, the odd last record alone); a followed
//                    record adds to word 2 and, unless it is a self-loop,
//                    unites its ends.  kSettled: first the bits of src and dst
//                    in the settled map (both gathers of every record of the
//                    iteration issued together); when both are set the record
//                    is skipped -- the two are in one tree and trees only
//                    merge, so a skip is always right.
//   k_comp_flatten : every entry in R becomes the root of its tree.
//   k_comp_major   : one workgroup: the majority label of kCompSample evenly
//                    spaced neurons of R (Afforest's sample).
//   k_comp_settled : bit n = (n in R and plane[n] == the majority label); every
//                    word of the map is written.
//   k_comp_merge   : unites n with planes[p][n] for every n in R and every p.
//   CLOSE          : k_comp_close_zero (the counters and words 3..6, the bins),
//                    k_comp_count (counters[label] += 1, equal labels
//                    aggregated along the wave with runs.h and, for the
//                    workgroup's first label, in LDS, before any global atomic),
//                    k_comp_stats (per root: the components, the singletons,
//                    the bins through an LDS histogram, the largest through one
//                    u64 atomicMax of size << 32 | ~label per workgroup),
//                    k_comp_sizes (SIZES: every neuron its label's counter),
//                    k_comp_final (words 0, 1, 4, 5).
#include "components.h"
#include "runs.h"
#include "scan.h"

#pragma clang fp contract(off)

namespace abnn {
namespace {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned long long u64;

struct CompArgs {
    const uint16_t* lo;
    const uint8_t* hi;
    const uint2* dw;
    u64* out;
    const uint32_t* settled;
    uint64_t k0, k1;  // records [k0, k1), k0 even
    uint32_t first, count;
    float w_lo, w_hi;
};

__device__ __forceinline__ uint32_t* plane_of(u64* out) { return reinterpret_cast<uint32_t*>(out + kCompPlaneAt); }

// a read of the plane: atomic for the compiler (never kept in a register), a plain cached load for the hardware
__device__ __forceinline__ uint32_t peek(const uint32_t* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ void give_up(u64* out, uint32_t code)
{
    (void)__hip_atomic_fetch_max(out + 7, (u64)code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x's tree, shortening the path on the way (path halving), or
// kCompNone after `cap` steps (never: every step decreases x).
__device__ __forceinline__ uint32_t find(uint32_t* plane, u64* out, uint32_t x, uint32_t cap)
{
    for (uint32_t steps = 0; steps <= cap; ++steps) {
        const uint32_t p = peek(plane + x);
        if (p == x) return x;
        const uint32_t g = peek(plane + p);
        if (g == p) return p;
        (void)__hip_atomic_fetch_min(plane + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = g;
    }
    give_up(out, kCompGaveUpFind);
    return kCompNone;
}

__device__ __forceinline__ void unite(uint32_t* plane, u64* out, uint32_t u, uint32_t v, uint32_t cap)
{
    // a failed hook lowers u, and v only ever moves down to its root: at most 2 * cap rounds
    for (uint64_t tries = 0; tries <= 2ull * cap; ++tries) {
        uint32_t ru = find(plane, out, u, cap), rv = find(plane, out, v, cap);
        if (ru == kCompNone || rv == kCompNone || ru == rv) return;
        if (ru < rv) {
            const uint32_t t = ru;
            ru = rv;
            rv = t;
        }
        uint32_t expected = ru;
        if (__hip_atomic_compare_exchange_strong(plane + ru, &expected, rv, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return;
        u = expected;  // fresh, and strictly below ru
        v = rv;
    }
    give_up(out, kCompGaveUpUnite);
}

__global__ __launch_bounds__(kCompPlaneThreads) void k_comp_begin(u64* out, uint32_t n_nrn, uint32_t first, uint32_t count)
{
    const uint32_t tid = threadIdx.x;
    if (blockIdx.x == 0)
        for (uint32_t j = tid; j < kCompPlaneAt; j += kCompPlaneThreads) out[j] = 0;
    u32x2* plane2 = reinterpret_cast<u32x2*>(out + kCompPlaneAt);
    const uint32_t n_words = (uint32_t)(((uint64_t)n_nrn + 1) >> 1);
    for (uint32_t j = blockIdx.x * kCompPlaneThreads + tid; j < n_words; j += gridDim.x * kCompPlaneThreads) {
        const uint32_t n0 = 2 * j, n1 = 2 * j + 1;  // n1 == n_nrn: the pad entry of an odd N_NRN, 0
        u32x2 v;
        v.x = (n0 - first < count) ? n0 : kCompNone;
        v.y = n1 >= n_nrn ? 0u : ((n1 - first < count) ? n1 : kCompNone);
        plane2[j] = v;
    }
}

// The settled map's word of neuron n, 0 when n is not in R (the load is issued
// all the same, from word 0, so that a lane's gathers go out together).
__device__ __forceinline__ uint32_t settled_word(const CompArgs& a, uint32_t n)
{
    const bool in = n - a.first < a.count;
    const uint32_t w = a.settled[in ? n >> 5 : 0u];
    return in ? w : 0u;
}

template <bool kWeight, bool kSettled>
__device__ __forceinline__ uint32_t link_record(const CompArgs& a, uint32_t* plane, uint32_t src, uint32_t dst, uint32_t wbits,
                                                uint32_t ws, uint32_t wd)
{
    if (src - a.first >= a.count || dst - a.first >= a.count) return 0;  // an absent record, a tombstone: dst above N_NRN
    if (kWeight) {
        const float w = __uint_as_float(wbits);
        if (!(w >= a.w_lo && w < a.w_hi)) return 0;  // NaN: not followed
    }
    if (src == dst) return 1;
    if (kSettled && ((ws >> (src & 31u)) & (wd >> (dst & 31u)) & 1u)) return 1;
    unite(plane, a.out, src, dst, a.count);
    return 1;
}

template <bool kWeight, bool kSettled>
__global__ __launch_bounds__(kCompThreads) void k_comp_link(CompArgs a)
{
    __shared__ u64 sums[kCompThreads / 64];
    constexpr uint32_t T = kCompThreads, U = kCompUnroll;
    uint32_t* plane = plane_of(a.out);
    const uint32_t tid = threadIdx.x;
    const RecordStream rs{reinterpret_cast<const u32x4*>(a.dw), a.dw, a.lo, a.hi};
    const uint64_t p_first = a.k0 >> 1, p_end = scan_pairs(a.k1);
    const uint64_t stride = (uint64_t)gridDim.x * (T * U);
    uint32_t followed = 0;
    for (uint64_t base = p_first + (uint64_t)blockIdx.x * (T * U); base < p_end; base += stride) {
        PairLoad<true, T, U> l;  // an absent record: a dst above N_NRN
        l.load(rs, base, a.k1, tid);
        uint32_t s0[U], s1[U], ws0[U], wd0[U], ws1[U], wd1[U];
#pragma unroll
        for (uint32_t k = 0; k < U; ++k) {
            s0[k] = l.src0(k);
            s1[k] = l.src1(k);
            if (kSettled) {
                ws0[k] = settled_word(a, s0[k]);
                wd0[k] = settled_word(a, l.v[k].x);
                ws1[k] = settled_word(a, s1[k]);
                wd1[k] = settled_word(a, l.v[k].z);
            } else {
                ws0[k] = wd0[k] = ws1[k] = wd1[k] = 0;
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < U; ++k) {
            followed += link_record<kWeight, kSettled>(a, plane, s0[k], l.v[k].x, l.v[k].y, ws0[k], wd0[k]);
            followed += link_record<kWeight, kSettled>(a, plane, s1[k], l.v[k].z, l.v[k].w, ws1[k], wd1[k]);
        }
    }
    const uint64_t wave_followed = wave_add((uint64_t)followed);
    if ((tid & 63u) == 0) sums[tid >> 6] = wave_followed;
    __syncthreads();
    if (tid == 0) {
        u64 s = 0;
        for (uint32_t w = 0; w < T / 64; ++w) s += sums[w];
        if (s) (void)__hip_atomic_fetch_add(a.out + 2, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(kCompPlaneThreads) void k_comp_flatten(u64* out, uint32_t first, uint32_t count)
{
    uint32_t* plane = plane_of(out);
    for (uint32_t j = blockIdx.x * kCompPlaneThreads + threadIdx.x; j < count; j += gridDim.x * kCompPlaneThreads) {
        const uint32_t n = first + j;
        const uint32_t r = find(plane, out, n, count);
        // the root is at or below every ancestor: after the minimum the entry IS the root
        if (r != kCompNone && r != n) (void)__hip_atomic_fetch_min(plane + n, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(kCompSample) void k_comp_major(const u64* out, uint32_t* major, uint32_t first, uint32_t count)
{
    __shared__ uint32_t label[kCompSample];
    __shared__ u64 best;
    const uint32_t* plane = reinterpret_cast<const uint32_t*>(out + kCompPlaneAt);
    const uint32_t tid = threadIdx.x;
    if (tid == 0) best = 0;
    const uint32_t mine = plane[first + (uint32_t)(((uint64_t)tid * count) / kCompSample)];
    label[tid] = mine;
    __syncthreads();
    uint32_t votes = 0;
    for (uint32_t j = 0; j < kCompSample; ++j) votes += label[j] == mine;
    // the most votes; among equals the smallest label
    (void)__hip_atomic_fetch_max(&best, (u64)votes << 32 | (uint32_t)~mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    if (tid == 0) {
        major[0] = ~(uint32_t)best;
        major[1] = (uint32_t)(best >> 32);
    }
}

__global__ __launch_bounds__(kCompPlaneThreads) void k_comp_settled(const u64* out, const uint32_t* major, u64* map,
                                                                    uint32_t n_nrn, uint32_t first, uint32_t count)
{
    const uint32_t* plane = reinterpret_cast<const uint32_t*>(out + kCompPlaneAt);
    const uint32_t m = major[0];
    const uint32_t n_round = (uint32_t)((((uint64_t)n_nrn + 63) >> 6) << 6);  // whole waves: every word is written
    for (uint32_t base = blockIdx.x * kCompPlaneThreads; base < n_round; base += gridDim.x * kCompPlaneThreads) {
        const uint32_t n = base + threadIdx.x;
        const bool set = n < n_round && n - first < count && plane[n] == m;
        const u64 bits = __ballot(set);
        if ((threadIdx.x & 63u) == 0 && n < n_round) map[n >> 6] = bits;
    }
}

__global__ __launch_bounds__(kCompPlaneThreads) void k_comp_merge(u64* out, const uint32_t* planes, uint32_t n_planes,
                                                                  uint64_t stride, uint32_t first, uint32_t count)
{
    uint32_t* plane = plane_of(out);
    for (uint32_t j = blockIdx.x * kCompPlaneThreads + threadIdx.x; j < count; j += gridDim.x * kCompPlaneThreads) {
        const uint32_t n = first + j;
        for (uint32_t p = 0; p < n_planes; ++p) {
            const uint32_t l = planes[p * stride + n];
            if (l - first < count && l != n) unite(plane, out, n, l, count);  // NONE, or no neuron of R: skipped
        }
    }
}

// ---- CLOSE ----------------------------------------------------------------------------------------

__global__ __launch_bounds__(kCompPlaneThreads) void k_comp_close_zero(u64* out, u64* counters2, uint32_t n_words)
{
    if (blockIdx.x == 0 && threadIdx.x < kCompPlaneAt) {
        const uint32_t j = threadIdx.x;
        if ((j >= 3 && j <= 6) || j >= kCompBinsAt) out[j] = 0;
    }
    for (uint32_t j = blockIdx.x * kCompPlaneThreads + threadIdx.x; j < n_words; j += gridDim.x * kCompPlaneThreads)
        counters2[j] = 0;
}

__global__ __launch_bounds__(kCompPlaneThreads) void k_comp_count(const u64* out, uint32_t* counters, uint32_t n_nrn,
                                                                  uint32_t first, uint32_t count)
{
    __shared__ uint32_t own;
    constexpr uint32_t T = kCompPlaneThreads;
    const u32x2* plane2 = reinterpret_cast<const u32x2*>(out + kCompPlaneAt);
    const uint32_t* plane = reinterpret_cast<const uint32_t*>(plane2);
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t n_pairs = (uint32_t)(((uint64_t)n_nrn + 1) >> 1);
    if (tid == 0) own = 0;
    // the label the workgroup's first neuron carries: after a flatten of a mostly connected graph, nearly every
    // neuron's -- its increments are summed in LDS and leave as one atomic
    uint32_t wg_key = kRunNone;
    {
        const uint64_t tile = 2ull * blockIdx.x * T;
        const uint64_t at = tile > first ? tile : first;
        if (at < (uint64_t)first + count) wg_key = plane[at];
    }
    __syncthreads();
    // uniform over the workgroup: scatter_runs needs every lane of the wave
    for (uint32_t base = blockIdx.x * T; base < n_pairs; base += gridDim.x * T) {
        const uint32_t j = base + tid;
        RunItem r0{kRunNone, 1}, r1{kRunNone, 1};
        if (j < n_pairs) {
            const u32x2 v = plane2[j];
            if (2 * j - first < count) r0.key = v.x;
            if (2 * j + 1 - first < count) r1.key = v.y;  // the pad entry of an odd N_NRN is not in R
        }
        scatter_runs(lane, r0, r1, [&](uint32_t key, uint64_t sum) {
            if (key == wg_key)
                __hip_atomic_fetch_add(&own, (uint32_t)sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else
                (void)__hip_atomic_fetch_add(counters + key, (uint32_t)sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        });
    }
    __syncthreads();
    if (tid == 0 && own) (void)__hip_atomic_fetch_add(counters + wg_key, own, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ u64 wave_max64(u64 v)
{
    for (int m = 32; m > 0; m >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, m), hi = __shfl_xor((uint32_t)(v >> 32), m);
        const u64 o = (u64)hi << 32 | lo;
        v = o > v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(kCompPlaneThreads) void k_comp_stats(u64* out, const uint32_t* counters, uint32_t first,
                                                                  uint32_t count)
{
    __shared__ uint32_t bins[ABNN_COMP_SIZE_BINS];
    __shared__ uint32_t roots, singles;
    __shared__ u64 best;
    constexpr uint32_t T = kCompPlaneThreads;
    const uint32_t* plane = reinterpret_cast<const uint32_t*>(out + kCompPlaneAt);
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    if (tid < ABNN_COMP_SIZE_BINS) bins[tid] = 0;
    if (tid == 0) {
        roots = singles = 0;
        best = 0;
    }
    __syncthreads();
    u64 top = 0;
    for (uint32_t base = blockIdx.x * T; base < count; base += gridDim.x * T) {
        const uint32_t j = base + tid;
        const uint32_t n = first + j;
        const bool root = j < count && plane[n] == n;
        const uint32_t s = root ? counters[n] : 0u;
        const u64 is_root = __ballot(root && s > 0), is_single = __ballot(root && s == 1);
        if (lane == 0 && is_root) {
            __hip_atomic_fetch_add(&roots, (uint32_t)__popcll(is_root), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (is_single)
                __hip_atomic_fetch_add(&singles, (uint32_t)__popcll(is_single), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        if (s > 1) {  // bin 0 holds exactly the components of size 1: it is word 6
            __hip_atomic_fetch_add(&bins[31 - __clz(s)], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        if (s > 0) {
            const u64 cand = (u64)s << 32 | (uint32_t)~n;
            top = cand > top ? cand : top;
        }
    }
    top = wave_max64(top);
    if (lane == 0 && top) (void)__hip_atomic_fetch_max(&best, top, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    if (tid < ABNN_COMP_SIZE_BINS) {
        const uint32_t c = tid == 0 ? singles : bins[tid];
        if (c) (void)__hip_atomic_fetch_add(out + kCompBinsAt + tid, (u64)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (tid == 64) {
        if (roots) (void)__hip_atomic_fetch_add(out + 3, (u64)roots, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (singles) (void)__hip_atomic_fetch_add(out + 6, (u64)singles, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // word 4 holds size << 32 | ~label until k_comp_final
        if (best) (void)__hip_atomic_fetch_max(out + 4, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// SIZES: the size plane holds the counters (a label's entry is its size already):
// every other neuron of R takes its label's.  Nothing reads an entry that another lane writes.
__global__ __launch_bounds__(kCompPlaneThreads) void k_comp_sizes(const u64* out, uint32_t* sizes, uint32_t first, uint32_t count)
{
    const uint32_t* plane = reinterpret_cast<const uint32_t*>(out + kCompPlaneAt);
    for (uint32_t j = blockIdx.x * kCompPlaneThreads + threadIdx.x; j < count; j += gridDim.x * kCompPlaneThreads) {
        const uint32_t n = first + j, l = plane[n];
        if (l != n && l - first < count) sizes[n] = sizes[l];
    }
}

__global__ void k_comp_final(u64* out, uint64_t n, uint32_t n_nrn)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const u64 packed = out[4];
    out[0] = n;
    out[1] = n_nrn;
    out[4] = packed >> 32;
    out[5] = (uint32_t)~(uint32_t)packed;
}

dim3 plane_grid(uint64_t items, uint32_t cus)
{
    constexpr uint64_t T = kCompPlaneThreads;
    return dim3((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(8ull * cus, (items + T - 1) / T)));
}

template <bool kSettled>
void launch_link(const CompArgs& a, bool weight, uint32_t cus, hipStream_t s)
{
    if (a.k1 <= a.k0) return;
    const uint64_t per_iter = 2ull * kCompThreads * kCompUnroll;
    const uint64_t iters = (a.k1 - a.k0 + per_iter - 1) / per_iter;
    const dim3 g((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(4ull * cus, iters))), b(kCompThreads);
    if (weight)
        hipLaunchKernelGGL((k_comp_link<true, kSettled>), g, b, 0, s, a);
    else
        hipLaunchKernelGGL((k_comp_link<false, kSettled>), g, b, 0, s, a);
}

}  // namespace

hipError_t launch_components_step(const SynArrays& syn, uint64_t n, const abnn_components_config& cfg, uint64_t n_nrn,
                                  uint32_t step, uint64_t* out_dev, const CompScratch& scratch, uint32_t path, uint32_t cus,
                                  hipStream_t s)
{
    u64* out = reinterpret_cast<u64*>(out_dev);
    const uint32_t nn = (uint32_t)n_nrn, first = cfg.first, count = cfg.count;
    const uint64_t plane_words = components_plane_words(n_nrn);
    const dim3 b(kCompPlaneThreads);
    cus = std::max(1u, cus);
    if (step == ABNN_COMP_BEGIN) {
        hipLaunchKernelGGL(k_comp_begin, plane_grid(plane_words, cus), b, 0, s, out, nn, first, count);
    } else if (step == ABNN_COMP_LINK) {
        CompArgs a{};
        a.lo = syn.lo;
        a.hi = syn.hi;
        a.dw = syn.dw;
        a.out = out;
        a.settled = scratch.settled;
        a.first = first;
        a.count = count;
        a.w_lo = cfg.w_lo;
        a.w_hi = cfg.w_hi;
        const bool weight = cfg.flags & ABNN_COMP_WEIGHT;
        const bool settled = path == 2 || (path == 0 && n >= kCompSettledMinPerNeuron * n_nrn);
        // the leading slice: even, so that the rest starts on a 16-B pair; at most half of the records
        const uint64_t slice = settled ? std::min<uint64_t>(kCompSlicePerNeuron * n_nrn, (n / 2) & ~1ull) : n;
        a.k0 = 0;
        a.k1 = slice;
        launch_link<false>(a, weight, cus, s);
        if (settled) {
            hipLaunchKernelGGL(k_comp_flatten, plane_grid(count, cus), b, 0, s, out, first, count);
            hipLaunchKernelGGL(k_comp_major, dim3(1), dim3(kCompSample), 0, s, out, scratch.major, first, count);
            hipLaunchKernelGGL(k_comp_settled, plane_grid(n_nrn, cus), b, 0, s, out, scratch.major,
                               reinterpret_cast<u64*>(scratch.settled), nn, first, count);
            a.k0 = slice;
            a.k1 = n;
            launch_link<true>(a, weight, cus, s);
        }
    } else if (step == ABNN_COMP_FLATTEN) {
        hipLaunchKernelGGL(k_comp_flatten, plane_grid(count, cus), b, 0, s, out, first, count);
    } else {  // ABNN_COMP_CLOSE
        const bool sizes = cfg.flags & ABNN_COMP_SIZES;
        uint32_t* counters = sizes ? reinterpret_cast<uint32_t*>(out + kCompPlaneAt + plane_words) : scratch.counts;
        hipLaunchKernelGGL(k_comp_close_zero, plane_grid(plane_words, cus), b, 0, s, out, reinterpret_cast<u64*>(counters),
                           (uint32_t)plane_words);
        hipLaunchKernelGGL(k_comp_count, plane_grid(plane_words, cus), b, 0, s, out, counters, nn, first, count);
        hipLaunchKernelGGL(k_comp_stats, plane_grid(count, cus), b, 0, s, out, counters, first, count);
        if (sizes) hipLaunchKernelGGL(k_comp_sizes, plane_grid(count, cus), b, 0, s, out, counters, first, count);
        hipLaunchKernelGGL(k_comp_final, dim3(1), dim3(64), 0, s, out, (uint64_t)n, nn);
    }
    return hipGetLastError();
}

hipError_t launch_components_merge(const abnn_components_config& cfg, uint64_t n_nrn, const uint32_t* planes_dev,
                                   uint32_t n_planes, uint64_t* out_dev, uint32_t cus, hipStream_t s)
{
    hipLaunchKernelGGL(k_comp_merge, plane_grid(cfg.count, std::max(1u, cus)), dim3(kCompPlaneThreads), 0, s,
                       reinterpret_cast<u64*>(out_dev), planes_dev, n_planes, 2 * components_plane_words(n_nrn), cfg.first,
                       cfg.count);
    return hipGetLastError();
}

}  // namespace abnn
