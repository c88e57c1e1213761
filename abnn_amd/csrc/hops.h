// hops.h -- reachability (hops.hip; abnn.h abnn_hops_*): a
// breadth-first search over a handle's records from a seed set, one streaming
// pass per hop against a one-bit-per-neuron frontier map, as the C-ABI
// implementation (capi.hip) launches it.
#pragma once

#include "engine.h"

namespace abnn {

constexpr int kHopsThreads = 512;          // k_hops_expand: 8 waves per workgroup
constexpr int kHopsFwdUnroll = 2;          // forward: 16-B lo + 8-B hi loads (8 records each) in flight per lane
constexpr int kHopsRevUnroll = 4;          // reverse: 16-B {dst, w} pair loads in flight per lane
constexpr int kHopsFrontierThreads = 256;  // k_hops_begin / k_hops_frontier

// k_hops_expand folds the frontier bitmap to this many u32 words in LDS (32 KiB:
// four workgroups per CU) when the frontier holds at most kHopsFoldMaxFrontier
// neurons (a folded bit is then set for at most one neuron in eight that is
// not in the frontier) or when the whole bitmap fits.
constexpr uint32_t kHopsFoldWords = 8192;
constexpr uint32_t kHopsFoldMaxFrontier = 32 * kHopsFoldWords / 8;

constexpr uint32_t kHopsAllFlags = ABNN_HOPS_REVERSE | ABNN_HOPS_WEIGHT;

// The checks of abnn_hops_words.
inline bool hops_config_ok(const abnn_hops_config* c, uint64_t n_nrn)
{
    if (!c || n_nrn == 0 || (c->flags & ~kHopsAllFlags)) return false;
    if (c->seed_count == 0 || (uint64_t)c->seed_first + c->seed_count > n_nrn) return false;
    if (c->max_hops < 1 || c->max_hops > ABNN_HOPS_MAX) return false;
    for (uint32_t r : c->reserved)
        if (r != 0) return false;
    uint32_t lo, hi;
    __builtin_memcpy(&lo, &c->w_lo, 4);
    __builtin_memcpy(&hi, &c->w_hi, 4);
    if (c->flags & ABNN_HOPS_WEIGHT) {
        if (!(c->w_lo < c->w_hi)) return false;  // false for a NaN bound too
    } else if (lo != 0 || hi != 0) {             // both +0.0f
        return false;
    }
    return true;
}

inline uint64_t hops_words(const abnn_hops_config* c, uint64_t n_nrn)
{
    if (!hops_config_ok(c, n_nrn)) return 0;
    return ABNN_HOPS_HEADER_WORDS + ((uint64_t)c->max_hops + 1) + (n_nrn + 1) / 2;
}

// u32 words of the frontier bitmap of n_nrn neurons
inline uint64_t hops_bitmap_words(uint64_t n_nrn) { return (n_nrn + 31) / 32; }

// One step (ABNN_HOPS_BEGIN or 0 .. max_hops) of the search over records
// [0, n) of `a` in out_dev (hops_words u64), in stream order on `s`; `bitmap`
// holds hops_bitmap_words(n_nrn) u32 and `cus` sizes the grids.  The config
// has passed hops_config_ok for n_nrn (< 2^32) and the step is valid.
hipError_t launch_hops_step(const SynArrays& a, uint64_t n, const abnn_hops_config& cfg, uint64_t n_nrn, uint32_t step,
                            uint64_t* out_dev, uint32_t* bitmap, uint32_t cus, hipStream_t s);

}  // namespace abnn
