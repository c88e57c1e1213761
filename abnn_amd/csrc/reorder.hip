// reorder.hip -- the record reorder (abnn.h abnn_reorder_*): the
// records of [0, n_syn) put into the stable order of a 33-bit key, a seeded
// shuffle, an order-preserving tombstone compaction, or a caller's permutation.
// Everything is launches in stream order; no workgroup waits for another (no
// look-back, no ticket, no residency assumption), so a reorder may sit between
// passes and beside other streams' kernels.  Every position is an integer
// prefix sum, never the return value of an atomic, so the order is stable and
// does not depend on the grid or on timing.
//
// The records are cut into tiles of kReorderTile and the tiles into at most
// kReorderMaxSegments SEGMENTS of consecutive tiles; a workgroup takes the tiles
// of one segment in order and carries its running offsets from tile to tile.
//
//   k_reorder_tombs     : tombstones per segment (one stream over {dst, w}).
//   k_reorder_tomb_scan : their exclusive prefix, the header words 0, 1 and 4.
//   k_reorder_keys<kSrc>: the stream of scan.h once more (kSrc: the key is src).
//       A stable partition: a live record's (k32, index) goes to pairs[0][its
//       rank among the live records], a tombstone's to [L + its rank among the
//       tombstones], L = n - T -- so the tombstone bit of the key is never
//       sorted: the radix passes below run over the first L pairs only.  The
//       rank inside a tile is the select's: ballots, mbcnt and an LDS prefix
//       over the tile's (load, wave) totals.  The AND and the OR of the live
//       keys go to the state words.
//   k_reorder_plan      : a radix pass whose digit is the same in every key (the
//       AND and the OR agree on its 8 bits: its global histogram has one
//       bucket) is skipped; which buffer each pass reads.
//   per radix pass (LSD, 8 bits; each returns at once when the pass is skipped):
//     k_reorder_count   : digit counts per segment, counts[digit * segs + seg];
//     k_reorder_scan    : their exclusive prefix in that (digit-major) order, one
//                         workgroup;
//     k_reorder_scatter : wave w of a workgroup owns 512 consecutive pairs of the
//         tile, slot s of lane l is pair w * 512 + s * 64 + l.  Slot by slot the
//         wave builds the match mask of every lane's digit from 8 ballots; the
//         first lane of a mask reads and advances the wave's own LDS counter of
//         that digit (plain loads and stores: the lanes of one wave, in program
//         order), so rank = counter + mbcnt(mask) is the element's rank among
//         the wave's earlier equal digits.  A prefix over the waves' counters
//         and the segment's running base give the position.
//   k_reorder_valid     : PERM: a one-bit-per-index map set with atomicOr; the
//       entries out of range or met before are COUNTED into word 3 (a count:
//       the same in any order).
//   k_reorder_pack      : a copy of the records as 12 B side by side {lo | hi <<
//       16, dst, w}: the move's gather is then ONE random access per record,
//       not one per stream (the move 31.8 ms against 69.7 ms at 1e9 records,
//       DESIGN.md §9).
//   k_reorder_move<kPerm>: new[k] = copy[origin[k]] into the records' own
//       arrays, two records per thread; counts `moved`, writes the origin plane.
//       It reads word 3 on the device and moves nothing when it is non-zero.
#include "reorder.h"
#include "scan.h"

#pragma clang fp contract(off)

namespace abnn {
namespace {

enum : uint32_t { kStAnd = 0, kStOr = 1, kStSkip = 2, kStSrc = 6 };  // state words: skip[4], src[5]
static_assert(kStSrc + kReorderPasses + 1 <= kReorderStateWords, "the state words");

struct ReorderArgs {
    RecordStream s;         // the live records
    uint32_t* copy;         // the move's source: their packed copy, 3 words per record {lo | hi << 16, dst, w}
    SynArrays dst;          // the move's destination: the live records
    uint2* pairs[2];
    uint32_t* counts;
    uint32_t* seg_tomb;
    uint32_t* state;
    const uint32_t* perm;
    unsigned long long* out;
    uint64_t n, syn_offset;
    uint32_t segs;       // workgroups of a tombs / keys / count / scatter launch
    uint32_t seg_tiles;  // record tiles per segment (tombs, keys)
    uint32_t pass, skip_on, want_origin;
    ReorderRule rule;
};

__device__ __forceinline__ uint32_t wave_scan(uint32_t v, uint32_t lane)  // inclusive
{
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

// exclusive prefix of v over a workgroup of kReorderScanThreads; lds holds one word per wave
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* lds, uint32_t tid, uint32_t* total)
{
    constexpr uint32_t W = kReorderScanThreads / 64;
    const uint32_t lane = tid & 63, wave = tid >> 6;
    const uint32_t incl = wave_scan(v, lane);
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    const uint32_t ws = wave_scan(lane < W ? lds[lane] : 0u, lane);
    const uint32_t before = wave ? __shfl(ws, wave - 1) : 0u;
    *total = __shfl(ws, W - 1);
    return before + incl - v;
}

__device__ __forceinline__ uint64_t live_count(const ReorderArgs& a) { return a.n - a.out[1]; }

using DwTile = PairLoad<false, kReorderThreads, kReorderUnroll, true>;
template <bool kSrc>
using KeyTile = PairLoad<kSrc, kReorderThreads, kReorderUnroll, true>;

__global__ __launch_bounds__(kReorderThreads) void k_reorder_tombs(ReorderArgs a)
{
    __shared__ uint32_t wave_tomb[kReorderThreads / 64];
    const uint32_t tid = threadIdx.x;
    const uint64_t tiles = (a.n + kReorderTile - 1) / kReorderTile;
    const uint64_t first = (uint64_t)blockIdx.x * a.seg_tiles, end = first + a.seg_tiles < tiles ? first + a.seg_tiles : tiles;
    uint32_t tomb = 0;
    for (uint64_t tile = first; tile < end; ++tile) {
        DwTile t;
        t.load(a.s, tile * (kReorderTile / 2), a.n, tid);
#pragma unroll
        for (uint32_t k = 0; k < kReorderUnroll; ++k)
            tomb += (t.valid0(k) && t.v[k].x == kAbsentDst) + (t.valid1(k) && t.v[k].z == kAbsentDst);
    }
    const uint32_t h[1] = {wave_add(tomb)};
    wave_words_to_lds(wave_tomb, h, tid);
    if (tid == 0) {
        uint32_t s = 0;
        for (uint32_t w = 0; w < kReorderThreads / 64; ++w) s += wave_tomb[w];
        a.seg_tomb[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(kReorderScanThreads) void k_reorder_tomb_scan(ReorderArgs a)
{
    __shared__ uint32_t lds[kReorderScanThreads / 64];
    const uint32_t tid = threadIdx.x;
    const uint32_t v = tid < a.segs ? a.seg_tomb[tid] : 0u;
    uint32_t total;
    const uint32_t before = block_excl_scan(v, lds, tid, &total);
    if (tid < a.segs) a.seg_tomb[tid] = before;
    if (tid == 0) {
        a.out[0] = a.n;
        a.out[1] = total;
        a.out[4] = a.syn_offset;
        a.state[kStAnd] = 0xFFFFFFFFu;
        a.state[kStOr] = 0u;
    }
}

__device__ __forceinline__ void put_pair(uint2* pairs, uint64_t pos, uint32_t key, uint64_t index)
{
    pairs[pos] = uint2{key, (uint32_t)index};
}

template <bool kSrc>
__global__ __launch_bounds__(kReorderThreads) void k_reorder_keys(ReorderArgs a)
{
    constexpr uint32_t U = kReorderUnroll, W = kReorderThreads / 64;
    static_assert(U * W <= 64, "the (load, wave) totals are scanned by one wave");
    __shared__ uint32_t totals[2][U * W];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t tiles = (a.n + kReorderTile - 1) / kReorderTile;
    const uint64_t first = (uint64_t)blockIdx.x * a.seg_tiles, end = first + a.seg_tiles < tiles ? first + a.seg_tiles : tiles;
    const uint64_t L = live_count(a);
    uint64_t tomb_before = a.seg_tomb[blockIdx.x];  // tombstones before the tile
    uint32_t k_and = 0xFFFFFFFFu, k_or = 0u, parity = 0;
    const unsigned long long below = (1ull << lane) - 1;
    uint2* pairs = a.pairs[0];
    for (uint64_t tile = first; tile < end; ++tile, parity ^= 1) {
        KeyTile<kSrc> t;
        t.load(a.s, tile * (kReorderTile / 2), a.n, tid);
        bool d0[U], d1[U];
        unsigned long long b0[U], b1[U];
#pragma unroll
        for (uint32_t k = 0; k < U; ++k) {
            d0[k] = t.valid0(k) && t.v[k].x == kAbsentDst;
            d1[k] = t.valid1(k) && t.v[k].z == kAbsentDst;
            b0[k] = __ballot(d0[k]);
            b1[k] = __ballot(d1[k]);
            if (lane == 0) totals[parity][k * W + wave] = __popcll(b0[k]) + __popcll(b1[k]);
        }
        __syncthreads();  // one per tile (the parity)
        const uint32_t before = wave_scan(lane < U * W ? totals[parity][lane] : 0u, lane);
        const uint32_t tile_tombs = __shfl(before, U * W - 1);
#pragma unroll
        for (uint32_t k = 0; k < U; ++k) {
            const uint32_t e = k * W + wave;
            const uint32_t groups = e ? __shfl(before, e - 1) : 0u;
            const uint64_t r0 = tomb_before + groups + __popcll(b0[k] & below) + __popcll(b1[k] & below);
            const uint64_t r1 = r0 + (d0[k] ? 1u : 0u);
            const uint64_t i0 = t.pair(k) << 1, i1 = i0 + 1;
            const uint32_t key0 = d0[k] ? 0u : reorder_key32(a.rule, t.src0(k), t.v[k].x, t.v[k].y, i0);
            const uint32_t key1 = d1[k] ? 0u : reorder_key32(a.rule, t.src1(k), t.v[k].z, t.v[k].w, i1);
            const uint64_t p0 = d0[k] ? L + r0 : i0 - r0, p1 = d1[k] ? L + r1 : i1 - r1;
            // p0, p1 < n always: the tombstone counts are of the same records
            if (t.valid1(k) && !d0[k] && !d1[k] && !(p0 & 1) && p1 < a.n) {  // two live neighbours, 16-B aligned
                *reinterpret_cast<u32x4*>(pairs + p0) = u32x4{key0, (uint32_t)i0, key1, (uint32_t)i1};
            } else {
                if (t.valid0(k) && p0 < a.n) put_pair(pairs, p0, key0, i0);
                if (t.valid1(k) && p1 < a.n) put_pair(pairs, p1, key1, i1);
            }
            if (t.valid0(k) && !d0[k]) k_and &= key0, k_or |= key0;
            if (t.valid1(k) && !d1[k]) k_and &= key1, k_or |= key1;
        }
        tomb_before += tile_tombs;
    }
    for (int m = 32; m > 0; m >>= 1) {
        k_and &= __shfl_xor(k_and, m);
        k_or |= __shfl_xor(k_or, m);
    }
    if (lane == 0) {
        if (k_and != 0xFFFFFFFFu) atomicAnd(a.state + kStAnd, k_and);
        if (k_or != 0u) atomicOr(a.state + kStOr, k_or);
    }
}

__global__ void k_reorder_plan(ReorderArgs a)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint64_t L = live_count(a);
    const uint32_t diff = a.state[kStAnd] ^ a.state[kStOr];
    uint32_t cur = 0;
    for (uint32_t p = 0; p < kReorderPasses; ++p) {
        const bool same = ((diff >> (8 * p)) & 0xFFu) == 0;
        const bool skip = L <= 1 || (a.skip_on && same);
        a.state[kStSkip + p] = skip ? 1u : 0u;
        a.state[kStSrc + p] = cur;
        if (!skip) cur ^= 1u;
    }
    a.state[kStSrc + kReorderPasses] = cur;
}

// the tiles [first, end) of pairs that workgroup `seg` takes in a radix pass over L pairs
__device__ __forceinline__ void radix_segment(const ReorderArgs& a, uint64_t L, uint64_t* first, uint64_t* end)
{
    const uint64_t tiles = (L + kReorderTile - 1) / kReorderTile;
    const uint64_t per = (tiles + a.segs - 1) / a.segs;
    const uint64_t f = (uint64_t)blockIdx.x * per;
    *first = f < tiles ? f : tiles;
    *end = f + per < tiles ? f + per : tiles;
}

__device__ __forceinline__ uint32_t digit_of(uint32_t key, uint32_t pass) { return (key >> (8 * pass)) & 0xFFu; }

__global__ __launch_bounds__(kReorderThreads) void k_reorder_count(ReorderArgs a)
{
    constexpr uint32_t S = kReorderSlots, T = kReorderThreads, kCopies = 32;
    __shared__ uint32_t hist[kReorderDigits * kCopies];
    if (a.state[kStSkip + a.pass]) return;
    const uint32_t tid = threadIdx.x;
    const uint2* in = a.pairs[a.state[kStSrc + a.pass]];
    const uint64_t L = live_count(a);
    uint64_t first, end;
    radix_segment(a, L, &first, &end);
    for (uint32_t i = tid; i < kReorderDigits * kCopies; i += T) hist[i] = 0;
    __syncthreads();
    for (uint64_t tile = first; tile < end; ++tile) {
        uint32_t key[S];
#pragma unroll
        for (uint32_t s = 0; s < S; ++s) {
            const uint64_t i = tile * kReorderTile + s * T + tid;
            key[s] = i < L ? in[i].x : 0u;
        }
#pragma unroll
        for (uint32_t s = 0; s < S; ++s) {
            const uint64_t i = tile * kReorderTile + s * T + tid;
            if (i < L) hist_add(hist, kCopies, tid & (kCopies - 1), digit_of(key[s], a.pass));
        }
    }
    __syncthreads();
    for (uint32_t d = tid; d < kReorderDigits; d += T) {  // every (digit, segment) word is written
        uint32_t sum = 0;
        for (uint32_t r = 0; r < kCopies; ++r) sum += hist[d * kCopies + ((r + tid) & (kCopies - 1))];
        a.counts[(uint64_t)d * a.segs + blockIdx.x] = sum;
    }
}

// One workgroup: thread t takes `per` consecutive words of the digit-major counts.
__global__ __launch_bounds__(kReorderScanThreads) void k_reorder_scan(ReorderArgs a)
{
    __shared__ uint32_t lds[kReorderScanThreads / 64];
    if (a.state[kStSkip + a.pass]) return;
    const uint32_t tid = threadIdx.x;
    const uint32_t E = kReorderDigits * a.segs, per = (E + kReorderScanThreads - 1) / kReorderScanThreads;
    const uint32_t lo = tid * per < E ? tid * per : E, hi = lo + per < E ? lo + per : E;
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += a.counts[i];
    uint32_t total;
    uint32_t run = block_excl_scan(sum, lds, tid, &total);
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t c = a.counts[i];
        a.counts[i] = run;
        run += c;
    }
}

__global__ __launch_bounds__(kReorderThreads) void k_reorder_scatter(ReorderArgs a)
{
    constexpr uint32_t S = kReorderSlots, T = kReorderThreads, W = T / 64, D = kReorderDigits;
    static_assert(D <= T, "one thread per digit");
    __shared__ uint32_t base[D];      // the segment's next position per digit
    __shared__ uint32_t wave_cnt[W * D];  // per wave: equal digits so far, then (after the prefix) those of earlier waves
    if (a.state[kStSkip + a.pass]) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t src = a.state[kStSrc + a.pass];
    const uint2* in = a.pairs[src];
    uint2* out = a.pairs[src ^ 1u];
    const uint64_t L = live_count(a);
    uint64_t first, end;
    radix_segment(a, L, &first, &end);
    if (tid < D) base[tid] = a.counts[(uint64_t)tid * a.segs + blockIdx.x];
    for (uint32_t i = tid; i < W * D; i += T) wave_cnt[i] = 0;
    __syncthreads();
    volatile uint32_t* mine = wave_cnt + wave * D;
    const unsigned long long below = (1ull << lane) - 1;
    for (uint64_t tile = first; tile < end; ++tile) {
        const uint64_t i0 = tile * kReorderTile + (uint64_t)wave * (S * 64) + lane;
        uint2 v[S];
        uint32_t rank[S];
#pragma unroll
        for (uint32_t s = 0; s < S; ++s) v[s] = i0 + s * 64 < L ? in[i0 + s * 64] : uint2{0u, 0u};
#pragma unroll
        for (uint32_t s = 0; s < S; ++s) {
            const bool valid = i0 + s * 64 < L;
            const uint32_t d = digit_of(v[s].x, a.pass);
            unsigned long long mask = __ballot(valid);
#pragma unroll
            for (uint32_t bit = 0; bit < 8; ++bit) {
                const bool one = (d >> bit) & 1u;
                const unsigned long long b = __ballot(one);
                mask &= one ? b : ~b;
            }
            const uint32_t leader = valid ? (uint32_t)__ffsll((long long)mask) - 1u : 0u;  // a valid lane is in its own mask
            uint32_t c = 0;
            if (valid && lane == leader) {
                c = mine[d];
                mine[d] = c + (uint32_t)__popcll(mask);
            }
            __builtin_amdgcn_wave_barrier();
            c = __shfl(c, leader);
            rank[s] = c + (uint32_t)__popcll(mask & below);
        }
        __syncthreads();
        uint32_t run = 0;  // thread d < D: the tile's count of digit d
        if (tid < D) {
            for (uint32_t w = 0; w < W; ++w) {
                const uint32_t c = wave_cnt[w * D + tid];
                wave_cnt[w * D + tid] = run;
                run += c;
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t s = 0; s < S; ++s) {
            if (i0 + s * 64 < L) {
                const uint32_t d = digit_of(v[s].x, a.pass);
                const uint64_t pos = (uint64_t)base[d] + wave_cnt[wave * D + d] + rank[s];
                if (pos < L) out[pos] = v[s];  // always: the counts are of the same pairs
            }
        }
        __syncthreads();
        if (tid < D) {
            base[tid] += run;
            for (uint32_t w = 0; w < W; ++w) wave_cnt[w * D + tid] = 0;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_reorder_valid(ReorderArgs a)
{
    __shared__ uint32_t wave_bad[4];
    uint32_t* map = reinterpret_cast<uint32_t*>(a.pairs[0]);  // zeroed by the launch: one bit per index
    uint32_t bad = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < a.n; k += (uint64_t)gridDim.x * 256) {
        const uint32_t p = a.perm[k];
        if (p >= a.n) {
            bad += 1;
        } else {
            const uint32_t bit = 1u << (p & 31u);
            bad += (atomicOr(map + (p >> 5), bit) & bit) ? 1u : 0u;
        }
    }
    const uint32_t h[1] = {wave_add(bad)};
    wave_words_to_lds(wave_bad, h, threadIdx.x);
    if (threadIdx.x == 0) {
        const unsigned long long s = (unsigned long long)wave_bad[0] + wave_bad[1] + wave_bad[2] + wave_bad[3];
        if (s) atomicAdd(a.out + 3, s);
    }
}

// The records' copy the move gathers from: {lo | hi << 16, dst, w} per record,
// 12 B side by side, so that the gather of a record is one access (three
// streams would be three random lines per record).  A lane writes its pair's
// 24 B as three 8-B stores.
__global__ __launch_bounds__(kReorderThreads) void k_reorder_pack(ReorderArgs a)
{
    const uint32_t tid = threadIdx.x;
    const uint64_t tiles = (a.n + kReorderTile - 1) / kReorderTile;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        PairLoad<true, kReorderThreads, kReorderUnroll, true> t;
        t.load(a.s, tile * (kReorderTile / 2), a.n, tid);
#pragma unroll
        for (uint32_t k = 0; k < kReorderUnroll; ++k) {
            const uint32_t c0 = (t.lo2[k] & 0xFFFFu) | (t.hi2[k] & 0xFFu) << 16;
            const uint32_t c1 = (t.lo2[k] >> 16) | ((t.hi2[k] >> 8) & 0xFFu) << 16;
            uint2* o = reinterpret_cast<uint2*>(a.copy + 6 * t.pair(k));  // 24 B per pair: 8-B aligned
            if (t.valid1(k)) {
                o[0] = uint2{c0, t.v[k].x};
                o[1] = uint2{t.v[k].y, c1};
                o[2] = uint2{t.v[k].z, t.v[k].w};
            } else if (t.valid0(k)) {
                uint32_t* w = a.copy + 6 * t.pair(k);
                w[0] = c0, w[1] = t.v[k].x, w[2] = t.v[k].y;
            }
        }
    }
}

template <bool kPerm>
__device__ __forceinline__ uint32_t origin_of(const ReorderArgs& a, const uint2* fin, uint64_t L, bool invalid, uint64_t k)
{
    if (kPerm) return invalid ? (uint32_t)k : a.perm[k];  // a valid perm: every entry is below n
    const uint32_t o = k < L ? fin[k].y : a.pairs[0][k].y;  // the tombstones' pairs never leave the first buffer
    return o < a.n ? o : (uint32_t)k;  // every index is below n; whatever happens, nothing outside the copy is read
}

template <bool kPerm>
__global__ __launch_bounds__(256) void k_reorder_move(ReorderArgs a)
{
    __shared__ uint32_t wave_moved[4];
    const bool invalid = kPerm && a.out[3] != 0;
    if (invalid && !a.want_origin) return;
    const uint64_t L = live_count(a);
    const uint2* fin = a.pairs[a.state[kStSrc + kReorderPasses]];
    uint2* plane = reinterpret_cast<uint2*>(a.out + ABNN_REORDER_HEADER_WORDS);
    const uint64_t pairs = scan_pairs(a.n);
    uint32_t moved = 0;
    for (uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x; q < pairs; q += (uint64_t)gridDim.x * 256) {
        const uint64_t k0 = q << 1, k1 = k0 + 1;
        const bool two = k1 < a.n;
        const uint32_t o0 = origin_of<kPerm>(a, fin, L, invalid, k0);
        const uint32_t o1 = two ? origin_of<kPerm>(a, fin, L, invalid, k1) : 0u;
        if (a.want_origin) plane[q] = uint2{o0, o1};
        if (invalid) continue;
        moved += (o0 != k0) + (two && o1 != k1);
        const uint32_t* g0 = a.copy + 3 * (uint64_t)o0;
        const uint32_t c0 = g0[0], d0 = g0[1], w0 = g0[2];
        if (two) {
            const uint32_t* g1 = a.copy + 3 * (uint64_t)o1;
            const uint32_t c1 = g1[0], d1 = g1[1], w1 = g1[2];
            reinterpret_cast<u32x4*>(a.dst.dw)[q] = u32x4{d0, w0, d1, w1};
            reinterpret_cast<uint32_t*>(a.dst.lo)[q] = (c0 & 0xFFFFu) | c1 << 16;
            reinterpret_cast<uint16_t*>(a.dst.hi)[q] = (uint16_t)((c0 >> 16) | (c1 >> 16) << 8);
        } else {
            a.dst.dw[k0] = uint2{d0, w0};
            a.dst.lo[k0] = (uint16_t)c0;
            a.dst.hi[hi_pos(k0)] = (uint8_t)(c0 >> 16);
        }
    }
    const uint32_t h[1] = {wave_add(moved)};
    wave_words_to_lds(wave_moved, h, threadIdx.x);
    if (threadIdx.x == 0) {
        const unsigned long long s = (unsigned long long)wave_moved[0] + wave_moved[1] + wave_moved[2] + wave_moved[3];
        if (s) atomicAdd(a.out + 2, s);
    }
}

#define REORDER_LAUNCH(kernel, grid, block)                        \
    do {                                                           \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, s, a); \
        e = hipGetLastError();                                     \
        if (e != hipSuccess) return e;                             \
    } while (0)

}  // namespace

hipError_t launch_reorder(const SynArrays& syn, uint64_t n, uint64_t syn_offset, const abnn_reorder_config& cfg,
                          const uint32_t* perm_dev, const ReorderScratch& scratch, uint64_t* out_dev, uint32_t blocks,
                          bool skip, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(out_dev, 0, ABNN_REORDER_HEADER_WORDS * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(scratch.state, 0, kReorderStateWords * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    const bool perm = cfg.key == ABNN_REORDER_PERM;
    ReorderArgs a{};
    a.s = record_stream(syn);
    a.copy = scratch.rec;
    a.dst = syn;
    a.pairs[0] = scratch.pairs[0];
    a.pairs[1] = scratch.pairs[1];
    a.counts = scratch.counts;
    a.seg_tomb = scratch.seg_tomb;
    a.state = scratch.state;
    a.perm = perm_dev;
    a.out = reinterpret_cast<unsigned long long*>(out_dev);
    a.n = n;
    a.syn_offset = syn_offset;
    a.skip_on = skip ? 1u : 0u;
    a.want_origin = (cfg.flags & ABNN_REORDER_ORIGIN) ? 1u : 0u;
    a.rule = reorder_rule(cfg, syn_offset);
    const uint64_t tiles = (n + kReorderTile - 1) / kReorderTile;
    uint64_t segs = std::min<uint64_t>(tiles, std::min<uint32_t>(std::max(1u, blocks), kReorderMaxSegments));
    const uint64_t seg_tiles = segs ? (tiles + segs - 1) / segs : 0;
    segs = seg_tiles ? (tiles + seg_tiles - 1) / seg_tiles : 0;  // none is empty
    a.segs = (uint32_t)segs;
    a.seg_tiles = (uint32_t)seg_tiles;
    if (n > 0) REORDER_LAUNCH(k_reorder_tombs, a.segs, kReorderThreads);
    REORDER_LAUNCH(k_reorder_tomb_scan, 1, kReorderScanThreads);
    if (n == 0) return hipSuccess;
    if (perm) {
        e = hipMemsetAsync(scratch.pairs[0], 0, ((n + 31) / 32) * sizeof(uint32_t), s);
        if (e != hipSuccess) return e;
        const uint32_t grid = (uint32_t)std::min<uint64_t>((n + 255) / 256, 4096);
        REORDER_LAUNCH(k_reorder_valid, grid, 256);
    } else {
        if (cfg.key == ABNN_REORDER_SRC)
            REORDER_LAUNCH(k_reorder_keys<true>, a.segs, kReorderThreads);
        else
            REORDER_LAUNCH(k_reorder_keys<false>, a.segs, kReorderThreads);
        REORDER_LAUNCH(k_reorder_plan, 1, 1);
        for (uint32_t p = 0; p < kReorderPasses; ++p) {
            a.pass = p;
            REORDER_LAUNCH(k_reorder_count, a.segs, kReorderThreads);
            REORDER_LAUNCH(k_reorder_scan, 1, kReorderScanThreads);
            REORDER_LAUNCH(k_reorder_scatter, a.segs, kReorderThreads);
        }
    }
    // the move gathers from a copy into the records' own arrays: the borrowed
    // pointers of abnn_state_ptrs stay valid
    REORDER_LAUNCH(k_reorder_pack, (uint32_t)std::min<uint64_t>(tiles, 8u * std::max(1u, blocks)), kReorderThreads);
    const uint32_t grid = (uint32_t)std::min<uint64_t>((scan_pairs(n) + 255) / 256, 16u * std::max(1u, blocks));
    if (perm)
        REORDER_LAUNCH(k_reorder_move<true>, grid, 256);
    else
        REORDER_LAUNCH(k_reorder_move<false>, grid, 256);
    return hipSuccess;
}

}  // namespace abnn
