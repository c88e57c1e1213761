// edit.hip -- the synapse edit (abnn.h abnn_edit_*): one
// streaming read-modify-write pass over the records of [0, n_syn).  One launch;
// no workgroup waits for another (no look-back, no ticket, no residency
// assumption), so an edit may run beside other streams' kernels.
//
//   k_edit<kSrc, kOp> : a persistent grid-stride stream over tiles of kEditTile
//       consecutive records; the stream is scan.h's (kEditUnroll loads in
//       flight; kSrc: a src range or SCALE_SRC).  The kernel writes through the
//       arrays it streams.  A lane applies the rule of edit.h to its two
//       records and
//       stores only what CHANGED: w alone (4 B), or the whole 16-B pair when
//       both records changed.  A kill stores the record's {dst, w} (8 B; 16 B
//       for both of a pair) and its own src code: the lo halfword, the hi byte
//       and, in random mode, src32 -- never a neighbour's bytes.  A tile is one
//       kCompactChunk, so the kills of a tile go to the structural update's
//       tally with one atomic per workgroup iteration.  The header counts are
//       per-lane integers, reduced per wave and per workgroup: one atomic per
//       workgroup and word at the end.
//   k_edit_factors : a grid-stride map over the strength words (edit_factor).
//
// Every count is an integer and every stored value a function of the record
// and its index alone, so the result does not depend on the grid or on timing.
#include "edit.h"
#include "scan.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace abnn {
namespace {

constexpr int kEditThreads = 512;  // 8 waves per workgroup
constexpr int kEditUnroll = 4;     // 16-B loads in flight per lane
constexpr uint32_t kEditTile = 2u * kEditThreads * kEditUnroll;  // records per workgroup iteration
static_assert(kEditTile == (uint32_t)kCompactChunk, "a tile's kills are one entry of the structural update's tally");
constexpr uint32_t kEditWaves = kEditThreads / 64;
constexpr int kFactorThreads = 256;

struct EditArgs {
    SynArrays syn;   // read as record_stream(syn), written in place; src32 in random mode only
    uint32_t* dead;   // the structural update's tally, or null
    const float* plane;
    unsigned long long* out;
    uint64_t n, tiles;
    uint32_t nt;  // non-temporal stores
    EditRule r;
};

template <typename T>
__device__ __forceinline__ void put(bool nt, T* p, T v)
{
    if (nt)
        __builtin_nontemporal_store(v, p);
    else
        *p = v;
}

// the tombstone of record i, as apply_event's prune branch leaves it: the src
// code of kSrcNone in the record's own halfword and byte, {dst = ~0, w}
__device__ __forceinline__ void kill_src(const EditArgs& a, uint64_t i)
{
    const uint32_t c = src_code(kSrcNone);
    a.syn.lo[i] = (uint16_t)c;
    a.syn.hi[hi_pos(i)] = (uint8_t)(c >> 16);
    if (a.syn.src32) a.syn.src32[i] = kSrcNone;
}

struct Counts {
    uint32_t tomb = 0, matched = 0, changed = 0, killed = 0, bad = 0;
};

// One record: match, the new bits (KILL: the old ones), the counts.  Returns
// whether the record is to be stored.
template <bool kSrc, uint32_t kOp>
__device__ __forceinline__ bool edit_one(const EditArgs& a, uint32_t src, uint32_t dst, uint32_t& wbits, uint64_t i,
                                         Counts& c)
{
    if (!edit_match<kSrc>(a.r, src, dst, wbits)) return false;
    ++c.matched;
    if (kOp == ABNN_EDIT_KILL) {
        ++c.killed;
        ++c.changed;
        return true;
    }
    uint32_t v = wbits;
    if (kOp == ABNN_EDIT_SCALE_DST || kOp == ABNN_EDIT_SCALE_SRC) {
        const uint32_t k = (kOp == ABNN_EDIT_SCALE_DST ? dst : src) - a.r.plane_first;
        if (k < a.r.plane_count) v = edit_value(a.r, wbits, a.plane[k], i);  // gathered from L2 / Infinity Cache
    } else {
        v = edit_value(a.r, wbits, 0.0f, i);
    }
    c.bad += edit_nonfinite(v);
    const bool changed = v != wbits;
    c.changed += changed;
    wbits = v;
    return changed;
}

template <bool kSrc, uint32_t kOp>
__global__ __launch_bounds__(kEditThreads) void k_edit(EditArgs a)
{
    constexpr uint32_t U = kEditUnroll;
    constexpr bool kKill = kOp == ABNN_EDIT_KILL;
    __shared__ uint32_t wave_kills[2][kEditWaves];
    __shared__ uint32_t wave_counts[kEditWaves * 5];
    const uint32_t tid = threadIdx.x;
    const RecordStream rs = record_stream(a.syn);
    const bool nt = a.nt != 0;
    Counts c;
    uint32_t parity = 0;
    for (uint64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x, parity ^= 1) {
        const uint64_t first_pair = tile * (kEditTile / 2);
        PairLoad<kSrc, kEditThreads, U, false> l;  // an absent record: a tombstone, no match
        l.load(rs, first_pair, a.n, tid);
        uint32_t tile_kills = 0;
#pragma unroll
        for (uint32_t k = 0; k < U; ++k) {
            const uint64_t p = l.pair(k);
            c.tomb += l.whole(k) ? (l.v[k].x == kEditTomb) + (l.v[k].z == kEditTomb) : 0u;
            uint32_t w0 = l.v[k].y, w1 = l.v[k].w;
            const uint64_t i = p << 1;
            const bool st0 = edit_one<kSrc, kOp>(a, l.src0(k), l.v[k].x, w0, i, c);
            const bool st1 = edit_one<kSrc, kOp>(a, l.src1(k), l.v[k].z, w1, i + 1, c);
            if (!(st0 || st1)) continue;  // a store only where a record changed (it exists: it matched)
            const uint32_t d0 = kKill && st0 ? kEditTomb : l.v[k].x, d1 = kKill && st1 ? kEditTomb : l.v[k].z;
            if (st0 && st1) {
                put(nt, reinterpret_cast<u32x4*>(a.syn.dw) + p, u32x4{d0, w0, d1, w1});
            } else if (kKill) {
                const uint64_t j = st0 ? i : i + 1;
                put(nt, reinterpret_cast<unsigned long long*>(a.syn.dw + j),
                    (unsigned long long)(st0 ? w0 : w1) << 32 | 0xFFFFFFFFull);  // {dst, w} as one 8-B store
            } else {
                const uint64_t j = st0 ? i : i + 1;
                put(nt, reinterpret_cast<uint32_t*>(a.syn.dw + j) + 1, st0 ? w0 : w1);
            }
            if (kKill) {
                if (st0) kill_src(a, i);
                if (st1) kill_src(a, i + 1);
                tile_kills += (uint32_t)st0 + (uint32_t)st1;
            }
        }
        if (kKill && a.dead) {  // uniform: the tile's kills into the tally with one atomic
            const uint32_t h[1] = {wave_add(tile_kills)};
            // one barrier per tile: the parity keeps the next tile's writes off this one's reads
            wave_words_to_lds(wave_kills[parity], h, tid);
            if (tid == 0) {
                uint32_t s = 0;
                for (uint32_t w = 0; w < kEditWaves; ++w) s += wave_kills[parity][w];
                if (s) atomicAdd(a.dead + tile, s);
            }
        }
    }
    if ((a.n & 1) && blockIdx.x == 0 && tid == 0) {
        const OddRecord r = odd_record<kSrc>(rs, a.n);
        const uint64_t i = a.n - 1;
        c.tomb += r.dst == kEditTomb;
        uint32_t w = r.w;
        if (edit_one<kSrc, kOp>(a, r.src, r.dst, w, i, c)) {
            if (kKill) {
                put(nt, reinterpret_cast<unsigned long long*>(a.syn.dw + i), (unsigned long long)w << 32 | 0xFFFFFFFFull);
                kill_src(a, i);
                if (a.dead) atomicAdd(a.dead + i / kCompactChunk, 1u);
            } else {
                put(nt, reinterpret_cast<uint32_t*>(a.syn.dw + i) + 1, w);
            }
        }
    }
    const uint32_t sums[5] = {wave_add(c.tomb), wave_add(c.matched), wave_add(c.changed), wave_add(c.killed),
                              wave_add(c.bad)};
    wave_words_to_lds(wave_counts, sums, tid);
    if (tid < 5) {
        unsigned long long s = 0;
        for (uint32_t w = 0; w < kEditWaves; ++w) s += wave_counts[w * 5 + tid];
        if (s) atomicAdd(a.out + 1 + tid, s);  // words 1..5
    }
    if (blockIdx.x == 0 && tid == 0) atomicAdd(a.out, (unsigned long long)a.n);  // zeroed before the launch
}

__global__ __launch_bounds__(kFactorThreads) void k_edit_factors(const uint64_t* strength, uint64_t count, float target,
                                                                  float f_lo, float f_hi, float* plane)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kFactorThreads + threadIdx.x; i < count; i += (uint64_t)gridDim.x * kFactorThreads)
        plane[i] = edit_factor(strength[i], target, f_lo, f_hi);
}

template <bool kSrc>
void launch_op(const EditArgs& a, uint32_t grid, hipStream_t s)
{
    const dim3 g(grid), t(kEditThreads);
    switch (a.r.op) {
    case ABNN_EDIT_SET: hipLaunchKernelGGL((k_edit<kSrc, ABNN_EDIT_SET>), g, t, 0, s, a); break;
    case ABNN_EDIT_AFFINE: hipLaunchKernelGGL((k_edit<kSrc, ABNN_EDIT_AFFINE>), g, t, 0, s, a); break;
    case ABNN_EDIT_SCALE_DST: hipLaunchKernelGGL((k_edit<kSrc, ABNN_EDIT_SCALE_DST>), g, t, 0, s, a); break;
    case ABNN_EDIT_SCALE_SRC: hipLaunchKernelGGL((k_edit<kSrc, ABNN_EDIT_SCALE_SRC>), g, t, 0, s, a); break;
    case ABNN_EDIT_DRAW: hipLaunchKernelGGL((k_edit<kSrc, ABNN_EDIT_DRAW>), g, t, 0, s, a); break;
    default: hipLaunchKernelGGL((k_edit<kSrc, ABNN_EDIT_KILL>), g, t, 0, s, a); break;
    }
}

}  // namespace

hipError_t launch_edit(const SynArrays& syn, uint64_t n, const EditRule& rule, const float* plane_dev, uint32_t* dead,
                       uint64_t* out_dev, uint32_t blocks, bool nt, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(out_dev, 0, ABNN_EDIT_HEADER_WORDS * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    EditArgs a{};
    a.syn = syn;
    a.dead = dead;
    a.plane = plane_dev;
    a.out = reinterpret_cast<unsigned long long*>(out_dev);
    a.n = n;
    a.tiles = (n + kEditTile - 1) / kEditTile;
    a.nt = nt ? 1u : 0u;
    a.r = rule;
    // the grid from the CU count (capi.hip: 4 workgroups, 32 waves, per CU, as the select); n == 0: the header alone
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::max(1u, blocks), a.tiles));
    // the src streams are read only where the rule needs them
    const bool src = rule.src_span != (rule.any ? 0u : 0xFFFFFFFFu) || rule.op == ABNN_EDIT_SCALE_SRC;
    if (src)
        launch_op<true>(a, grid, s);
    else
        launch_op<false>(a, grid, s);
    return hipGetLastError();
}

hipError_t launch_edit_factors(const uint64_t* strength_dev, uint64_t count, float target, float f_lo, float f_hi,
                               float* plane_dev, uint32_t blocks, hipStream_t s)
{
    if (count == 0) return hipSuccess;
    const uint64_t want = (count + kFactorThreads - 1) / kFactorThreads;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(want, std::max(1u, blocks));
    hipLaunchKernelGGL(k_edit_factors, dim3(grid), dim3(kFactorThreads), 0, s, strength_dev, count, target, f_lo, f_hi,
                       plane_dev);
    return hipGetLastError();
}

}  // namespace abnn
