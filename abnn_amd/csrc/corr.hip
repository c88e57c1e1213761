// corr.hip -- spike correlograms (abnn.h abnn_corr_*): lag
// histograms of the recorder's raster over a window of table rows.  The rule is
// corr.h's; every word of a result is an integer sum, so it depends on neither
// the grid nor the order nor the timing, and abnn_amd/corr.py restates it in
// numpy.  No workgroup waits for another and every loop is bounded by a count
// read once.
//
//   k_corr_rows<kStep> : workgroups take the window's rows by grid-stride.  K is
//       read from the recorder's device words and clamped to the pass capacity,
//       every row's offset + count to the raster capacity.
//       COUNT (every mode): per row the entries in A and in B -> tally[row]
//         (u32 pairs) and header words 0..3 and 7; for SYNAPSES also cnt[id] += 1
//         (u32 atomics without return) for every entry whose id is in A or B.
//       FILL (SYNAPSES): the row number of every such entry into its neuron's
//         list: rows[off[id] + cur[id]++].
//   k_corr_slabs : one lane per neuron.  A neuron with cnt > 0 takes a slab of
//       cnt entries of `rows` from ONE atomic cursor (no scan: the result is a
//       sum, so neither the order of the slabs nor of the entries inside a list
//       matters); a wave ballot writes every word of the has-a-list map.  A
//       slab that would end past the raster capacity (only a corrupted table,
//       whose clamped rows overlap, can ask for one) is refused: the neuron gets
//       no list and no bit.
//   k_corr_pop : one workgroup per lag: H[l + L] = sum_r cA[r] * cB[r + l] (u64).
//   k_corr_pairs : workgroups take rows p by grid-stride; a chunk of kCorrChunk
//       of row p's entries is compacted to its A-entries in LDS; for every row
//       q in [p - L, p + L] inside the window the lanes take q's B-entries and
//       add one (u64 atomic without return) per A-entry of the chunk.
//   k_corr_syn : the stream over the records, in the shape of
//       k_hops_expand forward: 16 B of lo and 8 B of hi = eight records per lane
//       and load, non-temporal, every load of an iteration issued before its
//       first use.  The src decodes from the 3-B code; the map is held in LDS
//       when it fits (N_NRN <= 2^18) and folded as hops folds its frontier when
//       it does not, the exact bit confirmed from global memory.  dw[k] is
//       gathered for the records whose src is in A (word 5 counts EVERY followed
//       record, and following needs dst and w); a followed record whose src and
//       dst both have lists is a double hit.  Double hits are staged in LDS
//       (kCorrQueue per workgroup iteration; past that a lane walks its own) and
//       drained after a barrier: a hit of at most kCorrLaneWalk pairs by one
//       lane, a longer one by a wave, whose lanes stride over the longer list
//       and each loop over the shorter one; pairs within L go to an LDS
//       histogram of 2L + 1 u64 bins, flushed once per workgroup with atomics.
//       The records that no whole 16-B load holds are read one at a time.
#include "corr.h"
#include "scan.h"

namespace abnn {
namespace {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned long long u64;

struct CorrArgs {
    CorrRule r;
    const unsigned long long* words;  // the recorder's device words
    const abnn_spike_pass* passes;
    const uint32_t* raster;
    uint64_t raster_cap;
    uint32_t pass_cap;
    CorrScratch s;
    u64* out;
    // k_corr_syn
    const uint16_t* lo;
    const uint8_t* hi;
    const uint2* dw;
    uint64_t n;
};

__device__ __forceinline__ void window_of(const CorrArgs& a, uint64_t* K, uint64_t* lo, uint64_t* hi)
{
    uint64_t k = a.words[3];
    k = k < a.pass_cap ? k : a.pass_cap;
    *K = k;
    corr_window(a.r, k, lo, hi);
}

__device__ __forceinline__ void add64(u64* p, u64 v)
{
    if (v) (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void lds_add64(u64* p, u64 v)
{
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

enum : int { kCount = 0, kFill = 1 };

template <int kStep>
__global__ __launch_bounds__(kCorrRowThreads) void k_corr_rows(CorrArgs a)
{
    __shared__ uint32_t s_a[kCorrRowThreads / 64], s_b[kCorrRowThreads / 64];
    constexpr uint32_t T = kCorrRowThreads;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const bool lists = a.r.mode == ABNN_CORR_SYNAPSES;
    uint64_t K, lo, hi;
    window_of(a, &K, &lo, &hi);
    u64 entries = 0, in_a = 0, in_b = 0;  // thread 0's
    for (uint64_t p = lo + blockIdx.x; p < hi; p += gridDim.x) {
        uint64_t off;
        uint32_t n;
        corr_row(a.passes[p], a.raster_cap, &off, &n);
        uint32_t na = 0, nb = 0;
        for (uint32_t i = tid; i < n; i += T) {
            const uint32_t id = a.raster[off + i];
            const bool ia = corr_in_a(a.r, id), ib = corr_in_b(a.r, id);
            if (kStep == kCount) {
                na += ia ? 1u : 0u;
                nb += ib ? 1u : 0u;
                if (lists && (ia || ib))
                    (void)__hip_atomic_fetch_add(a.s.cnt + id, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else if ((ia || ib) && ((a.s.map[id >> 5] >> (id & 31u)) & 1u)) {
                const uint32_t at = __hip_atomic_fetch_add(a.s.cur + id, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (at < a.s.cnt[id]) a.s.rows[a.s.off[id] + at] = (uint32_t)(p - lo);
            }
        }
        if (kStep == kCount) {  // p is uniform over the workgroup
            na = wave_add(na);
            nb = wave_add(nb);
            if (lane == 0) {
                s_a[wid] = na;
                s_b[wid] = nb;
            }
            __syncthreads();
            if (tid == 0) {
                uint32_t ta = 0, tb = 0;
                for (uint32_t w = 0; w < T / 64; ++w) {
                    ta += s_a[w];
                    tb += s_b[w];
                }
                a.s.tally[p] = make_uint2(ta, tb);
                entries += n;
                in_a += ta;
                in_b += tb;
            }
            __syncthreads();  // s_a / s_b are rewritten by the next row
        }
    }
    if (kStep == kCount && tid == 0) {
        add64(a.out + 1, entries);
        add64(a.out + 2, in_a);
        add64(a.out + 3, in_b);
        if (blockIdx.x == 0) {  // the only writer of words 0 and 7 (zeroed before)
            a.out[0] = hi - lo;
            a.out[7] = K;
        }
    }
}

__global__ __launch_bounds__(kCorrRowThreads) void k_corr_slabs(CorrArgs a)
{
    // whole waves: a lane past N_NRN carries no bit through the ballot
    const uint64_t n = (uint64_t)blockIdx.x * kCorrRowThreads + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    bool has = false;
    if (n < a.r.n_nrn) {
        const uint32_t c = a.s.cnt[n];
        uint32_t o = 0;
        if (c) {
            o = __hip_atomic_fetch_add(a.s.cursor, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            has = (uint64_t)o + c <= a.raster_cap;  // see the head of this file
        }
        a.s.off[n] = o;
        a.s.cur[n] = 0;
    }
    const unsigned long long ballot = __ballot(has);
    if (lane == 0 && n < a.r.n_nrn) {  // map holds corr_map_words: two words per wave that holds a neuron
        a.s.map[(n >> 5)] = (uint32_t)ballot;
        a.s.map[(n >> 5) + 1] = (uint32_t)(ballot >> 32);
    }
}

__global__ __launch_bounds__(kCorrRowThreads) void k_corr_pop(CorrArgs a)
{
    __shared__ u64 s_sum[kCorrRowThreads];
    constexpr uint32_t T = kCorrRowThreads;
    const uint32_t tid = threadIdx.x, bin = blockIdx.x;  // bin = l + L
    uint64_t K, lo, hi;
    window_of(a, &K, &lo, &hi);
    // rows p (A) and q = p + l (B), both in [lo, hi)
    const int64_t l = (int64_t)bin - (int64_t)a.r.L;
    const uint64_t rows = hi - lo, shift = (uint64_t)(l < 0 ? -l : l);
    u64 sum = 0;
    if (shift < rows) {
        const uint64_t p0 = l < 0 ? lo + shift : lo, count = rows - shift;
        for (uint64_t i = tid; i < count; i += T) {
            const uint64_t p = p0 + i, q = l < 0 ? p - shift : p + shift;
            sum += (u64)a.s.tally[p].x * (u64)a.s.tally[q].y;
        }
    }
    s_sum[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        for (uint32_t t = 1; t < T; ++t) sum += s_sum[t];
        a.out[ABNN_CORR_HEADER_WORDS + bin] = sum;
        add64(a.out + 4, sum);
    }
}

__global__ __launch_bounds__(kCorrRowThreads) void k_corr_pairs(CorrArgs a)
{
    __shared__ uint32_t s_ids[kCorrChunk];
    __shared__ uint32_t s_n;
    __shared__ u64 s_added;
    constexpr uint32_t T = kCorrRowThreads;
    const uint32_t tid = threadIdx.x;
    const uint64_t nb = 2ull * a.r.L + 1;
    u64* plane = a.out + ABNN_CORR_HEADER_WORDS;
    uint64_t K, lo, hi;
    window_of(a, &K, &lo, &hi);
    if (tid == 0) s_added = 0;
    u64 added = 0;
    for (uint64_t p = lo + blockIdx.x; p < hi; p += gridDim.x) {  // uniform over the workgroup
        if (a.s.tally[p].x == 0) continue;                          // no A-entry in row p
        uint64_t po;
        uint32_t pn;
        corr_row(a.passes[p], a.raster_cap, &po, &pn);
        const uint64_t q0 = p - lo > a.r.L ? p - a.r.L : lo, q1 = hi - p > a.r.L ? p + a.r.L + 1 : hi;
        for (uint32_t c0 = 0; c0 < pn; c0 += kCorrChunk) {
            __syncthreads();  // the last chunk's readers are done
            if (tid == 0) s_n = 0;
            __syncthreads();
            const uint32_t cn = pn - c0 < kCorrChunk ? pn - c0 : kCorrChunk;
            for (uint32_t i = tid; i < cn; i += T) {
                const uint32_t x = a.raster[po + c0 + i];
                if (corr_in_a(a.r, x)) s_ids[atomicAdd(&s_n, 1u)] = x - a.r.a_first;  // at most cn <= kCorrChunk
            }
            __syncthreads();
            const uint32_t na = s_n;
            if (na == 0) continue;
            for (uint64_t q = q0; q < q1; ++q) {
                if (a.s.tally[q].y == 0) continue;
                uint64_t qo;
                uint32_t qn;
                corr_row(a.passes[q], a.raster_cap, &qo, &qn);
                const uint64_t bin = (uint64_t)corr_bin(a.r.L, p, q);
                for (uint32_t j = tid; j < qn; j += T) {
                    const uint32_t y = a.raster[qo + j];
                    if (!corr_in_b(a.r, y)) continue;
                    const uint64_t col = (uint64_t)(y - a.r.b_first) * nb + bin, stride = (uint64_t)a.r.b_count * nb;
                    for (uint32_t e = 0; e < na; ++e)
                        (void)__hip_atomic_fetch_add(plane + s_ids[e] * stride + col, 1ull, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT);
                    added += na;
                }
            }
        }
    }
    __syncthreads();
    if (added) lds_add64(&s_added, added);
    __syncthreads();
    if (tid == 0) add64(a.out + 4, s_added);
}

// ---- SYNAPSES ------------------------------------------------------------------

struct SynShared {
    uint32_t fold[kCorrFoldWords];
    u64 hist[kCorrBins];
    uint2 queue[kCorrQueue];
    u64 followed, coupled;
    uint32_t qn;
};

// The map word of neuron n, 0 when n has no list (hops.hip frontier_word): the
// load is issued whether or not n is a neuron, so that a lane's gathers are all
// issued before the first one is used.
__device__ __forceinline__ uint32_t map_word(const CorrArgs& a, const uint32_t* fold, uint32_t n)
{
    bool may = n < a.r.n_nrn;
    may = may && ((fold[(n >> 5) & (kCorrFoldWords - 1u)] >> (n & 31u)) & 1u);
    const uint32_t w = a.s.map[may ? n >> 5 : 0u];
    return may ? w : 0u;
}

// The pairs of one record src -> dst (both have lists): lanes [lane0, lane0 +
// step, ...) over the longer list, each over the whole shorter one.  Returns
// the pairs this lane added.
__device__ __forceinline__ uint32_t walk(const CorrArgs& a, u64* hist, uint32_t src, uint32_t dst, uint32_t lane0,
                                         uint32_t step)
{
    const uint32_t os = a.s.off[src], ns = a.s.cnt[src], od = a.s.off[dst], nd = a.s.cnt[dst];
    const bool outer_src = ns >= nd;
    const uint32_t oo = outer_src ? os : od, no = outer_src ? ns : nd, oi = outer_src ? od : os, ni = outer_src ? nd : ns;
    uint32_t added = 0;
    for (uint32_t i = lane0; i < no; i += step) {
        const uint32_t xo = a.s.rows[oo + i];
        for (uint32_t j = 0; j < ni; ++j) {
            const uint32_t xi = a.s.rows[oi + j];
            const int32_t bin = outer_src ? corr_bin(a.r.L, xo, xi) : corr_bin(a.r.L, xi, xo);  // (pre's row, post's row)
            if (bin >= 0) {
                lds_add64(hist + bin, 1ull);
                ++added;
            }
        }
    }
    return added;
}

// `count` (<= 8) records from record `first` on, their src codes packed as the
// streams hold them.  Returns the followed records among them.
__device__ __forceinline__ uint32_t syn_group(const CorrArgs& a, SynShared& sh, uint64_t first, uint32_t count,
                                              const uint32_t (&lw)[4], const uint32_t (&hw)[2])
{
    uint32_t src[8], word[8];
    uint2 rec[8];
    bool in[8];
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
        src[j] = code_src((lw[j >> 1] >> (16u * (j & 1u))) & 0xFFFFu, (hw[j >> 2] >> (8u * (j & 3u))) & 0xFFu);
        in[j] = j < count && corr_in_a(a.r, src[j]);
        word[j] = map_word(a, sh.fold, in[j] ? src[j] : 0xFFFFFFFFu);
        rec[j] = a.dw[in[j] ? first + j : 0u];  // record 0 exists: n >= 1 here
    }
    uint32_t followed = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
        if (!in[j] || !corr_followed(a.r, src[j], rec[j].x, rec[j].y)) continue;
        ++followed;
        if (!((word[j] >> (src[j] & 31u)) & 1u)) continue;
        const uint32_t dst = rec[j].x;
        if (!((map_word(a, sh.fold, dst) >> (dst & 31u)) & 1u)) continue;
        const uint32_t slot = atomicAdd(&sh.qn, 1u);
        if (slot < kCorrQueue)
            sh.queue[slot] = make_uint2(src[j], dst);
        else if (walk(a, sh.hist, src[j], dst, 0u, 1u))  // the queue is full: this lane walks its own
            lds_add64(&sh.coupled, 1ull);
    }
    return followed;
}

// After a barrier: the staged double hits.  First a lane per hit: a hit whose
// two lists multiply to at most kCorrLaneWalk pairs is walked by its lane (most
// lists hold one or two rows, and a wave per such hit leaves 63 lanes idle);
// the longer ones are put back into the queue and walked one per wave.
__device__ __forceinline__ void drain(const CorrArgs& a, SynShared& sh)
{
    constexpr uint32_t kPerThread = kCorrQueue / kCorrThreads;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const uint32_t n = sh.qn < kCorrQueue ? sh.qn : kCorrQueue;
    uint2 mine[kPerThread];
    bool heavy[kPerThread];
#pragma unroll
    for (uint32_t k = 0; k < kPerThread; ++k) {
        const uint32_t i = tid + k * kCorrThreads;
        heavy[k] = false;
        if (i < n) {
            mine[k] = sh.queue[i];
            if ((uint64_t)a.s.cnt[mine[k].x] * a.s.cnt[mine[k].y] > kCorrLaneWalk)
                heavy[k] = true;
            else if (walk(a, sh.hist, mine[k].x, mine[k].y, 0u, 1u))
                lds_add64(&sh.coupled, 1ull);
        }
    }
    __syncthreads();  // every staged hit is in registers
    if (tid == 0) sh.qn = 0;
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kPerThread; ++k)
        if (heavy[k]) sh.queue[atomicAdd(&sh.qn, 1u)] = mine[k];  // at most n <= kCorrQueue
    __syncthreads();
    const uint32_t m = sh.qn;
    for (uint32_t i = wid; i < m; i += kCorrThreads / 64) {  // uniform over the wave
        const uint2 e = sh.queue[i];
        const uint32_t added = wave_add(walk(a, sh.hist, e.x, e.y, lane, 64u));
        if (lane == 0 && added) lds_add64(&sh.coupled, 1ull);
    }
    __syncthreads();
    if (tid == 0) sh.qn = 0;
    __syncthreads();
}

__global__ __launch_bounds__(kCorrThreads) void k_corr_syn(CorrArgs a)
{
    __shared__ SynShared sh;
    constexpr uint32_t T = kCorrThreads, U = kCorrUnroll;
    const uint32_t tid = threadIdx.x;
    const uint32_t nbins = 2u * a.r.L + 1u;
    // the map whole (bm_words <= kCorrFoldWords: word w in word w) or folded
    // (word w ORed into word w mod kCorrFoldWords); a record that passes the
    // fold is confirmed against the map.  Uniform over the grid.
    const uint32_t bm_words = (uint32_t)(((uint64_t)a.r.n_nrn + 31) >> 5);
    for (uint32_t i = tid; i < kCorrFoldWords; i += T) {
        uint32_t w = 0;
        for (uint32_t j = i; j < bm_words; j += kCorrFoldWords) w |= a.s.map[j];
        sh.fold[i] = w;
    }
    for (uint32_t i = tid; i < nbins; i += T) sh.hist[i] = 0;
    if (tid == 0) {
        sh.followed = 0;
        sh.coupled = 0;
        sh.qn = 0;
    }
    __syncthreads();

    const u32x4* lo4 = reinterpret_cast<const u32x4*>(a.lo);
    const u32x2* hi2 = reinterpret_cast<const u32x2*>(a.hi);
    const uint64_t n_groups = a.n >> 3;  // whole groups of eight records
    const uint64_t stride = (uint64_t)gridDim.x * (T * U);
    uint32_t followed = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * (T * U); base < n_groups; base += stride) {  // uniform over the workgroup
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
            if (g < n_groups) followed += syn_group(a, sh, 8 * g, 8u, lw, hw);
        }
        __syncthreads();
        drain(a, sh);
    }
    // the records no whole group holds, one at a time: nothing is read past record n - 1
    const uint32_t rest = (uint32_t)(a.n & 7u);
    if (rest && blockIdx.x == 0) {
        if (tid == 0) {
            uint32_t lw[4] = {0, 0, 0, 0}, hw[2] = {0, 0};
            for (uint32_t j = 0; j < rest; ++j) {
                const uint64_t k = 8 * n_groups + j;
                lw[j >> 1] |= (uint32_t)a.lo[k] << (16u * (j & 1u));
                hw[j >> 2] |= (uint32_t)a.hi[hi_pos(k)] << (8u * (j & 3u));
            }
            followed += syn_group(a, sh, 8 * n_groups, rest, lw, hw);
        }
        __syncthreads();
        drain(a, sh);
    }
    if (followed) lds_add64(&sh.followed, followed);
    __syncthreads();
    u64 sum = 0;
    for (uint32_t i = tid; i < nbins; i += T) {
        const u64 v = sh.hist[i];
        add64(a.out + ABNN_CORR_HEADER_WORDS + i, v);
        sum += v;
    }
    add64(a.out + 4, sum);
    if (tid == 0) {
        add64(a.out + 5, sh.followed);
        add64(a.out + 6, sh.coupled);
    }
}

}  // namespace

hipError_t launch_corr(const SynArrays& syn, uint64_t n, const abnn_corr_config& cfg, uint64_t n_nrn,
                       const SpikeRecorder& rec, const CorrScratch& scratch, uint64_t* out_dev, uint32_t cus,
                       hipStream_t s)
{
    cus = std::max(1u, cus);
    CorrArgs a{};
    a.r = corr_rule(cfg, n_nrn);
    a.words = rec.words;
    a.passes = rec.passes;
    a.raster = rec.raster;
    a.raster_cap = std::min<uint64_t>(rec.cfg.raster_capacity, scratch.raster_cap);
    a.pass_cap = std::min(rec.cfg.pass_capacity, scratch.pass_cap);
    a.s = scratch;
    a.out = reinterpret_cast<u64*>(out_dev);
    a.lo = syn.lo;
    a.hi = syn.hi;
    a.dw = syn.dw;
    a.n = n;
    hipError_t e = hipMemsetAsync(out_dev, 0, corr_words(&cfg) * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    const bool lists = cfg.mode == ABNN_CORR_SYNAPSES;
    if (lists) {
        if ((e = hipMemsetAsync(scratch.cnt, 0, n_nrn * sizeof(uint32_t), s)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(scratch.cursor, 0, 2 * sizeof(uint32_t), s)) != hipSuccess) return e;
    }
    const dim3 rt(kCorrRowThreads);
    const dim3 row_grid(std::max(1u, std::min(4u * cus, a.pass_cap)));
    hipLaunchKernelGGL(k_corr_rows<kCount>, row_grid, rt, 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (cfg.mode == ABNN_CORR_POP) {
        hipLaunchKernelGGL(k_corr_pop, dim3(2u * cfg.max_lag + 1u), rt, 0, s, a);
        return hipGetLastError();
    }
    if (cfg.mode == ABNN_CORR_PAIRS) {
        hipLaunchKernelGGL(k_corr_pairs, row_grid, rt, 0, s, a);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_corr_slabs, dim3((uint32_t)((n_nrn + kCorrRowThreads - 1) / kCorrRowThreads)), rt, 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_corr_rows<kFill>, row_grid, rt, 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (n == 0) return hipSuccess;
    // records per workgroup iteration; at least one workgroup: its first thread
    // takes the records that no whole 16-B load holds
    const uint64_t per_iter = 8ull * kCorrThreads * kCorrUnroll;
    const uint64_t iters = (n + per_iter - 1) / per_iter;
    const dim3 g((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(3ull * cus, iters))), b(kCorrThreads);
    hipLaunchKernelGGL(k_corr_syn, g, b, 0, s, a);
    return hipGetLastError();
}

}  // namespace abnn
