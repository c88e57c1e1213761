// index.hip -- the src index of the swept records and the per-pass event mask
// (index.h; DESIGN.md §5 "Indexed pass").
//
//   k_index_count / k_index_scan_* / k_index_scatter : the build, once per
//                graph: a count per neuron over the two src streams (runs of
//                one src along a wave's consecutive records add once, runs.h),
//                an exclusive scan in tiles, then every record's offset to its
//                neuron's list through a per-neuron cursor.
//   k_index_mark : per indexed pass, in front of k_gate: a delta mark.  The
//                mask persists from pass to pass and stands for the marked set
//                (index.h); the launch compares it with the pass's exact
//                recent-spike bitmap, ORs the lists of the neurons that enter
//                into the mask, AND-NOTs the lists of those that leave out of
//                it, and leaves marked set = bitmap.  Three dependent round
//                trips (bitmap words, row, off) and one atomic per entry of a
//                neuron that changed, entries of one wave-instruction and sign
//                that fall into one mask word merged first.  The lists above
//                kHeavyLen entries are cut into chunks at build time
//                (k_index_heavy_fill); each chunk has a workgroup of the same
//                launch, which returns when its neuron's bit did not change.
//   k_index_dirty : diagnostics, the mask's words that differ from another's.
//
// The build's two scans read the src streams alone (load_src_pair: 3 B per
// record).  scan.h's PairLoad is not used for them: it loads the pair's 16 B of
// {dst, w} whatever kSrc says, which the index never looks at -- 11 B per
// record instead of 3, 1.2 GB more per scan at config 3.  Its lane-to-record
// map is the same (lane l holds records 2 l and 2 l + 1 of a wave's 128), so
// runs.h applies as it does there; wave_add / wave_max are scan.h's.
#include "index.h"
#include "runs.h"
#include "scan.h"
#include "device.h"

namespace abnn {
namespace {

// Lists above kHeavyLen entries are heavy: the build cuts them into chunks of
// kHeavyChunk entries, each marked by a workgroup of its own (k_index_mark).
// The 256 stimulated inputs of the dense block are neighbours in the bitmap:
// walked by the wave that holds their words, their 65,536 entries took 1.8 ms.
constexpr uint32_t kHeavyLen = 128, kHeavyChunk = 1024;

// LDS written by some lanes of a wave and read by others of the same wave.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

// A wave's 128 consecutive records from `base` on: lane l holds records
// base + 2 l and base + 2 l + 1 (the arrays are padded by kDummyRecords, so the
// pair past the last record is there to read).  key: the record's src when it
// enters the index, else kRunNone.
struct SrcPair {
    uint32_t k0, k1;
};

__device__ __forceinline__ SrcPair load_src_pair(const SynArrays& a, uint64_t base, uint32_t lane, uint64_t events,
                                                 uint32_t n_nrn)
{
    const uint64_t p = (base >> 1) + lane;  // base is even
    const uint32_t lo2 = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(a.lo) + p);
    const uint32_t hi2 = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(a.hi) + p);
    const uint32_t s0 = code_src(lo2 & 0xFFFFu, hi2 & 0xFFu), s1 = code_src(lo2 >> 16, (hi2 >> 8) & 0xFFu);
    return SrcPair{2 * p < events && s0 < n_nrn ? s0 : kRunNone, 2 * p + 1 < events && s1 < n_nrn ? s1 : kRunNone};
}

__global__ __launch_bounds__(256) void k_index_count(SynArrays a, uint64_t events, uint32_t n_nrn, uint32_t* cnt)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6, waves = (uint64_t)gridDim.x * 4;
    for (uint64_t base = wave * 128; base < events; base += waves * 128) {  // wave-uniform
        const SrcPair k = load_src_pair(a, base, lane, events, n_nrn);
        scatter_runs(lane, RunItem{k.k0, 1ull}, RunItem{k.k1, 1ull},
                     [&](uint32_t key, uint64_t v) { atomicAdd(cnt + key, (uint32_t)v); });
    }
}

// Exclusive scan of one u32 per thread over a 1024-thread workgroup.
__device__ uint32_t block_scan_u32(uint32_t v, uint32_t* total, uint32_t* s_wave)
{
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint32_t inc = wave_incl_scan(v);
    if (lane == 63) s_wave[wid] = inc;
    __syncthreads();
    uint32_t before = 0, tot = 0;
    for (uint32_t w = 0; w < 16; ++w) {
        const uint32_t x = s_wave[w];
        before += w < wid ? x : 0u;
        tot += x;
    }
    __syncthreads();
    *total = tot;
    return before + inc - v;
}

// Tile t's count into part[t]; the largest degree into info[0].
__global__ __launch_bounds__(1024) void k_index_scan_a(const uint32_t* cnt, uint32_t n_nrn, uint32_t* part, uint32_t* info)
{
    __shared__ uint32_t s_wave[16];
    const uint64_t i0 = (uint64_t)blockIdx.x * kIndexTile + threadIdx.x * 4;
    uint32_t sum = 0, mx = 0, hc = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t c = i0 + j < n_nrn ? cnt[i0 + j] : 0u;
        sum += c;
        mx = c > mx ? c : mx;
        hc += c > kHeavyLen ? (c + kHeavyChunk - 1) / kHeavyChunk : 0u;
    }
    hc = wave_add(hc);
    if ((threadIdx.x & 63) == 0 && hc) atomicAdd(info + 2, hc);  // the heavy list's chunks
    uint32_t total;
    (void)block_scan_u32(sum, &total, s_wave);
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(info, mx);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// part[tiles] -> its exclusive scan in place; the total into part[tiles] and info[1].
__global__ __launch_bounds__(1024) void k_index_scan_b(uint32_t* part, uint32_t tiles, uint32_t* info)
{
    __shared__ uint32_t s_wave[16];
    uint32_t run = 0;
    for (uint32_t t0 = 0; t0 < tiles; t0 += 1024) {  // workgroup-uniform
        const uint32_t t = t0 + threadIdx.x;
        const uint32_t v = t < tiles ? part[t] : 0u;
        uint32_t total;
        const uint32_t ex = block_scan_u32(v, &total, s_wave);
        if (t < tiles) part[t] = run + ex;
        run += total;
    }
    if (threadIdx.x == 0) {
        part[tiles] = run;
        info[1] = run;
    }
}

// row[i] = cursor[i] = entries of the neurons below i (cursor holds the counts on entry).
__global__ __launch_bounds__(1024) void k_index_scan_c(uint32_t* cursor, uint32_t n_nrn, const uint32_t* part, uint32_t tiles,
                                                       uint32_t* row)
{
    __shared__ uint32_t s_wave[16];
    const uint64_t i0 = (uint64_t)blockIdx.x * kIndexTile + threadIdx.x * 4;
    uint32_t c[4], sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        c[j] = i0 + j < n_nrn ? cursor[i0 + j] : 0u;
        sum += c[j];
    }
    uint32_t total;
    uint32_t ex = part[blockIdx.x] + block_scan_u32(sum, &total, s_wave);
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        if (i0 + j < n_nrn) {
            row[i0 + j] = ex;
            cursor[i0 + j] = ex;
        }
        ex += c[j];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) row[n_nrn] = part[tiles];
}

__global__ __launch_bounds__(256) void k_index_scatter(SynArrays a, uint64_t events, uint32_t n_nrn, uint32_t* cursor,
                                                       uint32_t* off)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6, waves = (uint64_t)gridDim.x * 4;
    for (uint64_t base = wave * 128; base < events; base += waves * 128) {  // wave-uniform
        const SrcPair k = load_src_pair(a, base, lane, events, n_nrn);
        const uint64_t e0 = base + 2 * lane;
        if (k.k0 != kRunNone) {
            const uint32_t q = atomicAdd(cursor + k.k0, 1u);
            if (q < events) off[q] = (uint32_t)e0;  // (always: the counts are of the same records)
        }
        if (k.k1 != kRunNone) {
            const uint32_t q = atomicAdd(cursor + k.k1, 1u);
            if (q < events) off[q] = (uint32_t)(e0 + 1);
        }
    }
}

// Wave-converged: the lanes with act set (kClear: clear) bit o of the mask.
// Entries of one wave-instruction that share a mask word (a neuron whose
// records lie side by side: the dense input->output block, 32 to a word) would
// send as many same-address atomics; the lanes that share the first active
// lane's word are merged into one, for up to kMerge rounds while merging pays
// (a group of one ends it), as kernels.hip wave_set_next does for the next
// bitmap.  A call merges bits of one sign only: a wave-instruction that holds
// entries of entering and of leaving neurons takes two calls, and the OR and
// the AND-NOT that then meet in one word touch distinct bits and commute.
template <bool kClear>
__device__ __forceinline__ void wave_mask_apply(uint32_t* mask, bool act, uint32_t o)
{
    constexpr int kMerge = 8;
    auto apply = [&](uint32_t word, uint32_t bits) {
        if constexpr (kClear) (void)__hip_atomic_fetch_and(mask + word, ~bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else (void)__hip_atomic_fetch_or(mask + word, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    const uint32_t lane = threadIdx.x & 63, w = o >> 5, bit = 1u << (o & 31u);
    for (int it = 0; it < kMerge; ++it) {
        const uint64_t m = __ballot(act);
        if (m == 0) return;
        const uint32_t lead = (uint32_t)__builtin_ctzll(m);
        const uint32_t wl = (uint32_t)__builtin_amdgcn_readlane((int)w, (int)lead);
        const bool same = act && w == wl;
        if (__popcll(__ballot(same)) == 1) break;
        uint32_t bits = same ? bit : 0u;
#pragma unroll
        for (int x = 32; x > 0; x >>= 1) bits |= __shfl_xor(bits, x, 64);
        if (lane == lead) apply(wl, bits);
        act = act && !same;
    }
    if (act) apply(w, bit);
}

// Entry o of a neuron that enters the marked set (its bit is set) or leaves it
// (cleared); o past the sweep: neither.
__device__ __forceinline__ void wave_mask_delta(uint32_t* mask, uint64_t events, uint32_t o, bool leave)
{
    const bool valid = o < events;
    wave_mask_apply<false>(mask, valid && !leave, o);
    wave_mask_apply<true>(mask, valid && leave, o);
}

// The delta mark.  `old` is the marked set the mask stands for on entry, `now`
// this pass's exact bitmap; the launch moves the mask from the one to the
// other and leaves `next` = now (the host swaps old and next: a heavy
// workgroup reads old words that a light wave of the same launch would
// otherwise be overwriting).
// Light blocks (blockIdx < light): a wave takes kMarkWords words of the two
// bitmaps (512 neurons) and returns when they are equal.  The neurons of
// now & ~old (entering) and then those of old & ~now (leaving) go to an LDS
// list; up to 256 of them at a time read their row bounds (one round trip for
// all), wave scans of the list lengths flatten their entries, and the wave
// reads the entries four wave-instructions at a time (entry j belongs to the
// last neuron whose prefix is <= j: a search of the 256 prefixes in LDS; the
// neuron's place in the list tells whether it enters or leaves).  Lists above
// kHeavyLen entries are skipped here.
// Heavy blocks (the rest, one per chunk of the build's heavy list): the chunk's
// neuron's bit of both bitmaps -- equal: nothing to do, which is every
// stimulated input of a steady-state pass -- then its <= kHeavyChunk entries,
// four per lane.
// delta (may be null): {neurons entered, neurons left, entries set, entries
// cleared} of this launch: one atomic instruction per wave that found work,
// its lanes 0..3 each adding one non-zero counter (so up to four atomics, to
// one 16-B slot), into the wave's slot of kDeltaSlots.  The slots spread what
// would otherwise be every wave's atomics to one cache line, which serialise
// (profiles/ab_index_delta.txt).  The first workgroups zero delta_next, the
// next launch's block.
constexpr uint32_t kMarkWaves = 4, kMarkWords = 16, kMarkBatch = 256;

__global__ __launch_bounds__(kMarkWaves * 64) void k_index_mark(const uint32_t* now, const uint32_t* old, uint32_t* next,
                                                                uint32_t n_words, uint32_t n_nrn, const uint32_t* row,
                                                                const uint32_t* off, uint32_t* mask, uint64_t events,
                                                                const uint4* heavy, uint32_t light, uint32_t* delta,
                                                                uint32_t* delta_next)
{
    __shared__ uint16_t s_n[kMarkWaves][kMarkWords * 32];
    __shared__ uint32_t s_beg[kMarkWaves][kMarkBatch], s_pre[kMarkWaves][kMarkBatch];
    const uint32_t lane = threadIdx.x & 63, wid = wave_uniform(threadIdx.x >> 6);
    if (delta_next)
        for (uint32_t i = blockIdx.x * (kMarkWaves * 64) + threadIdx.x; i < 4 * kDeltaSlots; i += gridDim.x * (kMarkWaves * 64))
            delta_next[i] = 0u;
    if (delta) delta += 4u * ((blockIdx.x * kMarkWaves + wid) & (kDeltaSlots - 1u));
    if (blockIdx.x >= light) {  // workgroup-uniform
        const uint4 it = heavy[blockIdx.x - light];  // {neuron, first entry, entries, 0}
        const uint32_t was = (old[it.x >> 5] >> (it.x & 31u)) & 1u, is = (now[it.x >> 5] >> (it.x & 31u)) & 1u;
        if (was == is) return;
        const bool leave = was != 0u;
        uint32_t o[4];
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u) {
            const uint32_t j = (u * kMarkWaves + wid) * 64 + lane;
            o[u] = j < it.z ? off[it.y + j] : 0xFFFFFFFFu;
        }
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u) wave_mask_delta(mask, events, o[u], leave);
        if (delta && threadIdx.x == 0) atomicAdd(delta + (leave ? 3 : 2), it.z);
        return;
    }
    const uint32_t w0 = (blockIdx.x * kMarkWaves + wid) * kMarkWords;
    if (w0 >= n_words) return;  // wave-uniform
    const bool mine = lane < kMarkWords && w0 + lane < n_words;
    const uint32_t wnow = mine ? now[w0 + lane] : 0u, wold = mine ? old[w0 + lane] : 0u;
    if (mine) next[w0 + lane] = wnow;
    if (__ballot(wnow != wold) == 0) return;
    const uint32_t went = wnow & ~wold, wlev = wold & ~wnow;
    const uint32_t ce = (uint32_t)__builtin_popcount(went), ie = wave_incl_scan(ce);
    const uint32_t cl = (uint32_t)__builtin_popcount(wlev), il = wave_incl_scan(cl);
    const uint32_t n_ent = (uint32_t)__builtin_amdgcn_readlane((int)ie, 63);
    const uint32_t total = n_ent + (uint32_t)__builtin_amdgcn_readlane((int)il, 63);
    uint32_t q = ie - ce;
    for (uint32_t m = went; m; m &= m - 1u) s_n[wid][q++] = (uint16_t)(lane * 32u + (uint32_t)__builtin_ctz(m));
    q = n_ent + il - cl;
    for (uint32_t m = wlev; m; m &= m - 1u) s_n[wid][q++] = (uint16_t)(lane * 32u + (uint32_t)__builtin_ctz(m));
    wave_lds_sync();
    uint32_t set = 0, clr = 0;  // this lane's neurons' entries
    for (uint32_t c0 = 0; c0 < total; c0 += kMarkBatch) {  // wave-uniform
        uint32_t b[4], len[4];
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u) {
            const uint32_t i = c0 + u * 64 + lane;
            const uint32_t n = i < total ? w0 * 32u + s_n[wid][i] : 0xFFFFFFFFu;
            const bool vn = n < n_nrn;
            const uint32_t e = vn ? row[n + 1] : 0u;
            b[u] = vn ? row[n] : 0u;
            len[u] = e > b[u] && e - b[u] <= kHeavyLen ? e - b[u] : 0u;
            set += i < n_ent ? len[u] : 0u;
            clr += i < n_ent ? 0u : len[u];
        }
        uint32_t T = 0;
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u) {
            const uint32_t pre = wave_incl_scan(len[u]);
            s_beg[wid][u * 64 + lane] = b[u];
            s_pre[wid][u * 64 + lane] = T + pre - len[u];
            T += (uint32_t)__builtin_amdgcn_readlane((int)pre, 63);
        }
        wave_lds_sync();
        for (uint32_t j0 = 0; j0 < T; j0 += 256) {  // wave-uniform
            uint32_t o[4];
            bool leave[4];
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u) {
                const uint32_t j = j0 + u * 64 + lane;
                uint32_t lo = 0, hi = kMarkBatch;  // the last neuron of the batch with s_pre <= j (it holds entry j when j < T)
#pragma unroll
                for (int st = 0; st < 8; ++st) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (s_pre[wid][mid] <= j) lo = mid;
                    else hi = mid;
                }
                o[u] = j < T ? off[s_beg[wid][lo] + (j - s_pre[wid][lo])] : 0xFFFFFFFFu;
                leave[u] = c0 + lo >= n_ent;
            }
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u) wave_mask_delta(mask, events, o[u], leave[u]);
        }
        wave_lds_sync();  // the next batch overwrites s_beg / s_pre
    }
    if (delta) {  // lanes 0..3: one atomic instruction
        set = wave_add(set);
        clr = wave_add(clr);
        const uint32_t v = lane == 0 ? n_ent : lane == 1 ? total - n_ent : lane == 2 ? set : clr;
        if (lane < 4 && v) atomicAdd(delta + lane, v);
    }
}

// The build's heavy list: a thread per neuron; a list above kHeavyLen entries
// becomes chunks {neuron, first entry, entries, 0} at slots taken from *cursor.
__global__ __launch_bounds__(256) void k_index_heavy_fill(const uint32_t* row, uint32_t n_nrn, uint4* heavy, uint32_t cap,
                                                          uint32_t* cursor)
{
    const uint64_t n = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= n_nrn) return;
    const uint32_t b = row[n], len = row[n + 1] - b;
    if (len <= kHeavyLen) return;
    const uint32_t nch = (len + kHeavyChunk - 1) / kHeavyChunk, slot = atomicAdd(cursor, nch);
    for (uint32_t c = 0; c < nch && slot + c < cap; ++c)
        heavy[slot + c] = make_uint4((uint32_t)n, b + c * kHeavyChunk, min(kHeavyChunk, len - c * kHeavyChunk), 0u);
}

__global__ __launch_bounds__(256) void k_index_dirty(const uint32_t* mask, const uint32_t* want, uint64_t words,
                                                     unsigned long long* out)
{
    uint32_t n = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (uint64_t)gridDim.x * 256) n += mask[i] != want[i];
    n = wave_add(n);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(out, (unsigned long long)n);
}

}  // namespace

hipError_t launch_index_build(const SynArrays& syn, uint64_t events, uint64_t n_nrn, uint32_t* row, uint32_t* cursor,
                              uint32_t* part, uint32_t* off, uint32_t* info, uint32_t cus, hipStream_t s)
{
    const uint32_t tiles = (uint32_t)index_tiles(n_nrn), nn = (uint32_t)n_nrn;
    hipError_t e = hipMemsetAsync(cursor, 0, (n_nrn + 1) * 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(info, 0, 4 * 4, s);
    if (e != hipSuccess) return e;
    // 128 records per wave and step; 8 workgroups of 4 waves per CU, no more than there are steps
    const uint64_t steps = (events + 511) / 512;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(1u, cus) * 8, steps));
    hipLaunchKernelGGL(k_index_count, dim3(grid), dim3(256), 0, s, syn, events, nn, cursor);
    hipLaunchKernelGGL(k_index_scan_a, dim3(tiles), dim3(1024), 0, s, cursor, nn, part, info);
    hipLaunchKernelGGL(k_index_scan_b, dim3(1), dim3(1024), 0, s, part, tiles, info);
    hipLaunchKernelGGL(k_index_scan_c, dim3(tiles), dim3(1024), 0, s, cursor, nn, part, tiles, row);
    hipLaunchKernelGGL(k_index_scatter, dim3(grid), dim3(256), 0, s, syn, events, nn, cursor, off);
    return hipGetLastError();
}

hipError_t launch_index_heavy(const uint32_t* row, uint64_t n_nrn, uint4* heavy, uint32_t chunks, uint32_t* info,
                              hipStream_t s)
{
    if (chunks == 0 || n_nrn == 0) return hipSuccess;
    hipLaunchKernelGGL(k_index_heavy_fill, dim3((uint32_t)((n_nrn + 255) / 256)), dim3(256), 0, s, row, (uint32_t)n_nrn, heavy,
                       chunks, info + 3);
    return hipGetLastError();
}

hipError_t launch_index_mark(const uint32_t* bitmap, const uint32_t* marked, uint32_t* marked_next, uint32_t n_words,
                             uint64_t n_nrn, const uint32_t* row, const uint32_t* off, uint32_t* mask, uint64_t events,
                             const uint4* heavy, uint32_t chunks, uint32_t* delta, uint32_t* delta_next, hipStream_t s)
{
    if (n_words == 0) return hipSuccess;
    const uint32_t per = kMarkWaves * kMarkWords, light = (n_words + per - 1) / per;
    hipLaunchKernelGGL(k_index_mark, dim3(light + chunks), dim3(kMarkWaves * 64), 0, s, bitmap, marked, marked_next, n_words,
                       (uint32_t)n_nrn, row, off, mask, events, heavy, light, delta, delta_next);
    return hipGetLastError();
}

hipError_t launch_index_dirty(const uint32_t* mask, const uint32_t* want, uint64_t words, unsigned long long* out,
                              hipStream_t s)
{
    hipError_t e = hipMemsetAsync(out, 0, 8, s);
    if (e != hipSuccess) return e;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(2048, (words + 255) / 256));
    hipLaunchKernelGGL(k_index_dirty, dim3(grid), dim3(256), 0, s, mask, want, words, out);
    return hipGetLastError();
}

}  // namespace abnn
