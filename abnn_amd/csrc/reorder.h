// reorder.h -- the record reorder (reorder.hip; abnn.h abnn_reorder_*, DESIGN.md
// §9): a stable key sort, a seeded shuffle, a tombstone compaction or a caller's
// permutation of a handle's records.  The rule lives here ONCE, as __host__
// __device__ inlines: the kernels (reorder.hip) and abnn_reorder_host (capi.hip)
// share the config check and the key, so they cannot drift apart.  The rule's
// part of this header needs nothing but abnn.h, so a plain C++ compiler can
// build it (tests/cpp/reorder_host_test.cpp).
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/abnn/abnn.h"

#if defined(__HIPCC__)
#define ABNN_REORDER_HD __host__ __device__
#else
#define ABNN_REORDER_HD
#endif

namespace abnn {

constexpr uint32_t kReorderTomb = 0xFFFFFFFFu;  // the tombstone's dst
constexpr uint32_t kReorderAllFlags = ABNN_REORDER_DESCENDING | ABNN_REORDER_ORIGIN;
constexpr uint64_t kReorderMaxRecords = 1ull << 32;  // local indices are u32

// The checks of abnn_reorder_words that need no record count.
inline bool reorder_config_ok(const abnn_reorder_config* c)
{
    if (!c || c->key > ABNN_REORDER_PERM || (c->flags & ~kReorderAllFlags)) return false;
    for (uint32_t r : c->reserved)
        if (r != 0) return false;
    if ((c->flags & ABNN_REORDER_DESCENDING) && c->key > ABNN_REORDER_W) return false;
    if (c->key != ABNN_REORDER_RANDOM && c->seed != 0) return false;
    return true;
}

inline uint64_t reorder_words(const abnn_reorder_config* c, uint64_t n)
{
    if (!reorder_config_ok(c) || n > kReorderMaxRecords) return 0;
    return ABNN_REORDER_HEADER_WORDS + ((c->flags & ABNN_REORDER_ORIGIN) ? (n + 1) / 2 : 0);
}

// splitmix64_at of the graph builder (graph.h)
ABNN_REORDER_HD inline uint64_t reorder_splitmix64_at(uint64_t seed, uint64_t k)
{
    uint64_t z = seed + (k + 1u) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// A config that passed the checks, as the key reads it.
struct ReorderRule {
    uint32_t key, flip;  // flip: 0xFFFFFFFF with DESCENDING, else 0
    uint64_t draw_key, syn_offset;
};

inline ReorderRule reorder_rule(const abnn_reorder_config& c, uint64_t syn_offset)
{
    return ReorderRule{c.key, (c.flags & ABNN_REORDER_DESCENDING) ? 0xFFFFFFFFu : 0u, c.seed ^ ABNN_REORDER_KEY,
                       syn_offset};
}

// k32 of the LIVE record {src, dst, w bits} at local index k (a tombstone's is 0).
ABNN_REORDER_HD inline uint32_t reorder_key32(const ReorderRule& r, uint32_t src, uint32_t dst, uint32_t wbits, uint64_t k)
{
    uint32_t v = 0;
    if (r.key == ABNN_REORDER_SRC) v = src;
    else if (r.key == ABNN_REORDER_DST) v = dst;
    else if (r.key == ABNN_REORDER_W) v = wbits ^ ((wbits >> 31) ? 0xFFFFFFFFu : 0x80000000u);
    else if (r.key == ABNN_REORDER_RANDOM) v = (uint32_t)(reorder_splitmix64_at(r.draw_key, r.syn_offset + k) >> 32);
    return v ^ r.flip;
}

// The rule over n host records in place (abnn_reorder_host): the config has
// passed reorder_words(&c, n) != 0, perm is non-null exactly with PERM, out
// holds reorder_words(&c, n) u64.
inline void reorder_host(const abnn_reorder_config& c, uint64_t syn_offset, abnn_synapse* rec, uint64_t n,
                         const uint32_t* perm, uint64_t* out)
{
    const ReorderRule r = reorder_rule(c, syn_offset);
    const uint64_t words = reorder_words(&c, n);
    for (uint64_t i = 0; i < words; ++i) out[i] = 0;
    out[0] = n;
    out[4] = syn_offset;
    for (uint64_t k = 0; k < n; ++k) out[1] += rec[k].dst == kReorderTomb;
    std::vector<uint32_t> origin(n);
    for (uint64_t k = 0; k < n; ++k) origin[k] = (uint32_t)k;
    if (c.key == ABNN_REORDER_PERM) {
        std::vector<bool> seen(n, false);
        for (uint64_t k = 0; k < n; ++k) {
            if (perm[k] >= n || seen[perm[k]]) out[3] += 1;
            else seen[perm[k]] = true;
        }
        if (out[3] == 0)
            for (uint64_t k = 0; k < n; ++k) origin[k] = perm[k];
    } else {
        std::vector<uint64_t> key(n);
        for (uint64_t k = 0; k < n; ++k) {
            uint32_t wbits;
            __builtin_memcpy(&wbits, &rec[k].w, 4);
            key[k] = rec[k].dst == kReorderTomb ? 1ull << 32 : reorder_key32(r, rec[k].src, rec[k].dst, wbits, k);
        }
        std::stable_sort(origin.begin(), origin.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    }
    std::vector<abnn_synapse> old(rec, rec + n);
    for (uint64_t k = 0; k < n; ++k) {
        rec[k] = old[origin[k]];
        rec[k].pad = 0.0f;
        out[2] += origin[k] != k;
    }
    if (c.flags & ABNN_REORDER_ORIGIN)
        for (uint64_t k = 0; k < n; ++k) out[ABNN_REORDER_HEADER_WORDS + k / 2] |= (uint64_t)origin[k] << (32 * (k & 1));
}

}  // namespace abnn

#if defined(__HIPCC__)
#include "engine.h"

namespace abnn {

constexpr int kReorderThreads = 512;   // 8 waves per workgroup
constexpr int kReorderUnroll = 4;      // keys pass: 16-B record loads in flight per lane
constexpr uint32_t kReorderSlots = 8;  // radix passes: 8-B (key, index) loads in flight per lane
// Elements per tile: what one workgroup loads in one iteration -- 4096 records
// in the keys pass, 4096 (key, index) pairs in a radix pass.  Mirrored by
// abnn_amd/reorder.py TILE.
constexpr uint32_t kReorderTile = 4096;
static_assert(kReorderTile == 2u * kReorderThreads * kReorderUnroll, "a tile of records is one workgroup iteration");
static_assert(kReorderTile == kReorderThreads * kReorderSlots, "a tile of pairs is one workgroup iteration");
constexpr uint32_t kReorderDigits = 256;  // 8 bits per radix pass
constexpr uint32_t kReorderPasses = 4;
// The most segments (workgroups of a keys or radix launch): a segment is a run
// of consecutive tiles that one workgroup takes in order, so the per-digit
// counts are kReorderDigits x segments u32, scanned by one workgroup.
constexpr uint32_t kReorderMaxSegments = 1024;
constexpr int kReorderScanThreads = 1024;
constexpr uint32_t kReorderStateWords = 16;  // u32: {and, or, skip[4], src[5], ...} (reorder.hip)

// A handle's reorder scratch (capi.hip allocates it for syn_capacity and frees it).
struct ReorderScratch {
    uint2* pairs[2] = {nullptr, nullptr};  // (k32, index), ping-pong; pairs[0] doubles as PERM's bit map
    uint32_t* rec = nullptr;               // the records' copy the move gathers from: 3 words per record, packed
                                           // {lo | hi << 16, dst, w} so that a gather is one access, not three
    uint32_t* counts = nullptr;            // [kReorderDigits * kReorderMaxSegments] per (digit, segment), then their prefix
    uint32_t* seg_tomb = nullptr;          // [kReorderMaxSegments + 1] tombstones per segment, then their prefix
    uint32_t* state = nullptr;             // [kReorderStateWords]
    uint64_t capacity = 0;                 // records the buffers hold
};

// Reorders records [0, n) of `a` by cfg (local record k has global index
// syn_offset + k) and fills out_dev (reorder_words u64), all in stream order on
// `s`; at most `blocks` workgroups per launch.  perm_dev: PERM's n u32.  The
// config has passed reorder_words(&cfg, n) != 0 and n <= scratch.capacity.
// skip: leave out the radix passes whose digit is the same for every record.
hipError_t launch_reorder(const SynArrays& a, uint64_t n, uint64_t syn_offset, const abnn_reorder_config& cfg,
                          const uint32_t* perm_dev, const ReorderScratch& scratch, uint64_t* out_dev, uint32_t blocks,
                          bool skip, hipStream_t s);

}  // namespace abnn
#endif
