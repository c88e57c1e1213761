// select.h -- the synapse select (select.hip; abnn.h abnn_select_*, DESIGN.md
// §9): an ordered stream compaction of a handle's records -- the records that
// match a src / dst / weight rule, in record order and with their indices, into
// a caller-sized device buffer -- as the C-ABI implementation (capi.hip)
// launches it.
#pragma once

#include "engine.h"

namespace abnn {

constexpr int kSelectThreads = 512;  // 8 waves per workgroup
constexpr int kSelectUnroll = 4;     // 16-B loads in flight per lane
// Records per tile: the consecutive records one workgroup loads in one
// iteration (two per 16-B load).  The count launch leaves one match count per
// tile, the emit launch skips the tiles without a match.  Mirrored by
// abnn_amd/select.py TILE.
constexpr uint32_t kSelectTile = 4096;
static_assert(kSelectTile == 2u * kSelectThreads * kSelectUnroll, "a tile is one workgroup iteration");
constexpr int kSelectScanThreads = 1024;
constexpr uint32_t kSelectScanSegment = 16384;  // tiles per k_select_scan workgroup (16 counts per thread)
constexpr uint32_t kSelectEmitChunk = 64;  // tiles whose counts an emit workgroup looks at together

constexpr uint32_t kSelectAllFlags = ABNN_SELECT_ANY | ABNN_SELECT_WEIGHT;

inline uint64_t select_tiles(uint64_t n) { return (n + kSelectTile - 1) / kSelectTile; }
// u32 entries of the tile-count scratch for `n` records (whole 16-B loads for the scan)
inline uint64_t select_count_words(uint64_t n) { return (select_tiles(n) + 3) & ~3ull; }

// The checks of abnn_select_words (everything that needs no handle).
inline bool select_config_ok(const abnn_select_config* c)
{
    if (!c || (c->flags & ~kSelectAllFlags) || c->reserved != 0) return false;
    if ((uint64_t)c->src_first + c->src_count > (1ull << 32)) return false;  // a range that wraps u32
    if ((uint64_t)c->dst_first + c->dst_count > (1ull << 32)) return false;
    if ((c->flags & ABNN_SELECT_ANY) && c->src_count == 0 && c->dst_count == 0) return false;
    uint32_t lo, hi;
    __builtin_memcpy(&lo, &c->w_lo, 4);
    __builtin_memcpy(&hi, &c->w_hi, 4);
    if (c->flags & ABNN_SELECT_WEIGHT) {
        if (!(c->w_lo < c->w_hi)) return false;  // false for a NaN bound too
    } else if (lo != 0 || hi != 0) {             // both +0.0f
        return false;
    }
    return true;
}

inline uint64_t select_words(const abnn_select_config* c, uint64_t capacity)
{
    if (!select_config_ok(c)) return 0;
    if (capacity > (~0ull - ABNN_SELECT_HEADER_WORDS) / 3) return 0;
    return ABNN_SELECT_HEADER_WORDS + 3 * capacity;
}

// The handle's scratch: one u32 match count and one u64 output offset per tile
// (select_count_words(capacity) and select_tiles(capacity) entries).
struct SelectScratch {
    uint32_t* counts = nullptr;
    uint64_t* offsets = nullptr;
};

// Zeroes the 8 header words of out_dev and fills it with the select of records
// [0, n) of `a` (indices offset by syn_offset), all in stream order on `s`;
// the count and the emit launch have at most `blocks` workgroups.  Plane entries at and past `written` are not written.
// The config has passed select_config_ok and the range checks.
hipError_t launch_select(const SynArrays& a, uint64_t n, uint64_t syn_offset, const abnn_select_config& cfg,
                         uint64_t capacity, const SelectScratch& scratch, uint64_t* out_dev, uint32_t blocks,
                         hipStream_t s);

}  // namespace abnn
