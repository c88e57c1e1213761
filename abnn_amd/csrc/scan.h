// scan.h -- the record stream of the census-style kernels (census, degree,
// select, edit, snapshot diff, the reverse pass of hops), written
// once.  Internal, like engine.h; device inlines and a few host inlines, no
// translation unit of its own.
//
// The stream.  Records are taken as 16-B pairs: lane `tid` of a workgroup of T
// threads holds, for load k of an iteration, pair p = first_pair + k * T + tid =
// records 2p and 2p + 1.  All U loads of an iteration are issued before the
// first use, non-temporal (a scan reads every record once).  The two src
// streams -- the pair's 4 B of lo words and 2 B of hi bytes -- are loaded only
// in the kSrc instantiation.  When n is odd the last pair holds one record; it
// is loaded alone (8 B, 2 B, 1 B), so nothing is read past record n - 1.  With
// kOdd (degree, hops reverse) that happens inside load(), and the kernel has no
// block for "the record no pair holds"; without it (select, edit: the branch
// costs their emit and store loops registers that cost occupancy,
// profiles/scan_refactor_resources.txt) the kernel takes odd_record() after
// its loop.  A record that is absent (at or past n) reads as {dst = kAbsentDst,
// w = 0}: a tombstone to every match rule.  A kernel that COUNTS tombstones
// asks valid0 / valid1 or whole.  k_census and k_diff read a RecordStream with
// loops of their own (their speed rests on those loops' schedule).
#pragma once

#include <algorithm>

#include "engine.h"

namespace abnn {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kAbsentDst = 0xFFFFFFFFu;  // the tombstone's dst (= ABNN_HOPS_UNREACHED)
// a workgroup's LDS counters are u32: no workgroup scans more records than this
constexpr uint64_t kScanMaxPerWg = 1ull << 31;

__device__ __forceinline__ uint32_t wave_add(uint32_t v)
{
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__device__ __forceinline__ uint64_t wave_add(uint64_t v)
{
    for (int m = 32; m > 0; m >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, m), hi = __shfl_xor((uint32_t)(v >> 32), m);
        v += (uint64_t)hi << 32 | lo;
    }
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

struct RecordStream {
    const u32x4* dw4;  // the {dst, w} stream, two records per element
    const uint2* dw;
    const uint16_t* lo;
    const uint8_t* hi;
};

__host__ __device__ inline RecordStream record_stream(const SynArrays& s)
{
    return RecordStream{reinterpret_cast<const u32x4*>(s.dw), s.dw, s.lo, s.hi};
}

// pairs that hold a record of [0, n): the last one holds one record when n is odd
__host__ __device__ inline uint64_t scan_pairs(uint64_t n) { return (n + 1) >> 1; }

// One iteration's loads of one lane.
template <bool kSrc, uint32_t T, uint32_t U, bool kOdd = true>
struct PairLoad {
    u32x4 v[U];  // {dst0, w0, dst1, w1}
    uint32_t lo2[U], hi2[U];
    uint64_t p0, n;

    __device__ __forceinline__ void load(const RecordStream& s, uint64_t first_pair, uint64_t n_records, uint32_t tid)
    {
        p0 = first_pair + tid;
        n = n_records;
#pragma unroll
        for (uint32_t k = 0; k < U; ++k) {
            const uint64_t p = pair(k);
            v[k] = u32x4{kAbsentDst, 0u, kAbsentDst, 0u};
            lo2[k] = hi2[k] = 0;
            if (whole(k)) {
                v[k] = __builtin_nontemporal_load(s.dw4 + p);
                if (kSrc) {
                    lo2[k] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(s.lo) + p);
                    hi2[k] = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(s.hi) + p);
                }
            } else if (kOdd && 2 * p < n) {  // the last record of an odd n
                const uint2 r = s.dw[2 * p];
                v[k].x = r.x;
                v[k].y = r.y;
                if (kSrc) {
                    lo2[k] = s.lo[2 * p];
                    hi2[k] = s.hi[hi_pos(2 * p)];
                }
            }
        }
    }
    __device__ __forceinline__ uint64_t pair(uint32_t k) const { return p0 + k * T; }
    // Both records of load k exist: all there is to ask without kOdd.  One test, written as the loop each
    // form came from wrote it: the other spelling costs that loop registers (scan_refactor_resources.txt).
    __device__ __forceinline__ bool whole(uint32_t k) const { return kOdd ? 2 * pair(k) + 1 < n : pair(k) < n >> 1; }
    __device__ __forceinline__ bool valid0(uint32_t k) const { return kOdd ? 2 * pair(k) < n : whole(k); }
    __device__ __forceinline__ bool valid1(uint32_t k) const { return whole(k); }
    __device__ __forceinline__ uint32_t src0(uint32_t k) const { return kSrc ? code_src(lo2[k] & 0xFFFFu, hi2[k] & 0xFFu) : 0u; }
    __device__ __forceinline__ uint32_t src1(uint32_t k) const { return kSrc ? code_src(lo2[k] >> 16, (hi2[k] >> 8) & 0xFFu) : 0u; }
};

// The last record of an odd n, for a kernel that keeps it out of its loop
// (PairLoad<..., false>): one thread of the grid takes it.
struct OddRecord {
    uint32_t src, dst, w;  // of record n - 1
};

template <bool kSrc>
__device__ __forceinline__ OddRecord odd_record(const RecordStream& s, uint64_t n)
{
    const uint64_t i = n - 1;
    const uint2 r = s.dw[i];
    return OddRecord{kSrc ? code_src(s.lo[i], s.hi[hi_pos(i)]) : 0u, r.x, r.y};
}

// The grid of a scan whose workgroups keep lds_words u32 of LDS and take
// records_per_iter records per iteration: as many workgroups per CU as the LDS
// leaves room for (160 KiB per CU), at most 4 (32 waves); no more than there
// are iterations; and enough that none scans more than max_per_wg records.
inline uint32_t scan_grid(uint64_t n, uint64_t records_per_iter, uint32_t lds_words, uint32_t cus, uint64_t max_per_wg)
{
    const uint32_t per_cu = std::max(1u, std::min<uint32_t>(4u, (160u * 1024u) / (lds_words * 4u)));
    const uint64_t iters = (n + records_per_iter - 1) / records_per_iter;
    uint64_t grid = std::min<uint64_t>((uint64_t)std::max(1u, cus) * per_cu, iters);
    const uint64_t max_iters = max_per_wg / records_per_iter;
    if ((iters + grid - 1) / grid > max_iters) grid = (iters + max_iters - 1) / max_iters;
    return (uint32_t)grid;
}

// The bank-spread histogram.  A distribution that falls into a few bins (the
// generated graph's weights: 6-7 of 64; a constant: one) would serialise a
// single LDS histogram on those addresses, so a workgroup keeps `copies` of it,
// interleaved as hist[bin * copies + (lane & (copies - 1))]: with 32 copies the
// 32 lanes an LDS atomic services together always hit 32 different banks; with
// fewer, equal bins from different lanes still spread over `copies` banks.
constexpr uint32_t kHistLdsWords = 16384;  // 64 KiB of u32 counters per workgroup
constexpr uint32_t kHistMaxCopies = 32;

// the most copies (a power of two) that fit: 4096 bins -> 4, <= 512 -> 32
inline uint32_t hist_copies(uint32_t bins)
{
    uint32_t r = kHistMaxCopies;
    while (r > 1 && (uint64_t)bins * r > kHistLdsWords) r >>= 1;
    return r;
}

__device__ __forceinline__ void hist_add(uint32_t* hist, uint32_t copies, uint32_t copy, uint32_t bin)
{
    __hip_atomic_fetch_add(&hist[bin * copies + copy], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// after a barrier: a thread sums the copies of its bins, starting at its own
// copy so that the lanes of a wave read different banks; zero bins are skipped
__device__ __forceinline__ void hist_flush(const uint32_t* hist, uint32_t bins, uint32_t copies, uint32_t tid, uint32_t T,
                                           unsigned long long* out)
{
    for (uint32_t b = tid; b < bins; b += T) {
        uint32_t s = 0;
        for (uint32_t r = 0; r < copies; ++r) s += hist[b * copies + ((r + tid) & (copies - 1))];
        if (s) atomicAdd(out + b, (unsigned long long)s);
    }
}

// The header epilogue's first half: lane 0 of wave w writes the wave's K sums
// to lds[w * K ..], then a barrier.  The combine over the waves is the kernel's.
template <uint32_t K, typename W>
__device__ __forceinline__ void wave_words_to_lds(W* lds, const W (&h)[K], uint32_t tid)
{
    if ((tid & 63) == 0) {
#pragma unroll
        for (uint32_t j = 0; j < K; ++j) lds[(tid >> 6) * K + j] = h[j];
    }
    __syncthreads();
}

}  // namespace abnn
