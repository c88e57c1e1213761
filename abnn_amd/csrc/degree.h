// degree.h -- the neuron degree census (degree.hip; abnn.h abnn_degree_*,
// DESIGN.md §9): one streaming pass over a handle's records that counts, per
// neuron of a range, the live records that leave it and that enter it, and sums
// their weights in fixed point, as the C-ABI implementation (capi.hip) launches it.
#pragma once

#include "engine.h"

namespace abnn {

constexpr int kDegreeThreads = 512;  // 8 waves per workgroup
constexpr int kDegreeUnroll = 4;     // 16-B loads in flight per lane
// Ranges of at most this many neurons take the narrow path (accumulators in
// LDS), longer ones the wide path (atomics into the result).  Mirrored by
// abnn_amd/degree.py NARROW_MAX.
constexpr uint32_t kDegreeNarrowMax = 4096;
// a narrow launch's accumulators fit this; a range whose four planes do not
// (more than 2730 neurons) is scanned once per direction
constexpr uint32_t kDegreeLdsBytes = 64 * 1024;

constexpr uint32_t kDegreeAll = ABNN_DEG_OUT | ABNN_DEG_IN | ABNN_DEG_OUT_W | ABNN_DEG_IN_W;

// The checks of abnn_degree_words; *count = the neurons of the range.
inline bool degree_config_ok(const abnn_degree_config* c, uint64_t n_nrn, uint64_t* count)
{
    if (!c || n_nrn == 0 || c->what == 0 || (c->what & ~kDegreeAll)) return false;
    for (uint32_t r : c->reserved)
        if (r != 0) return false;
    if (c->count == 0 && c->first != 0) return false;
    if ((uint64_t)c->first + c->count > n_nrn) return false;
    if (count) *count = c->count ? (uint64_t)c->count : n_nrn;
    return true;
}

inline uint64_t degree_words(const abnn_degree_config* c, uint64_t n_nrn)
{
    uint64_t m = 0;
    if (!degree_config_ok(c, n_nrn, &m)) return 0;
    return ABNN_DEGREE_HEADER_WORDS + (uint64_t)__builtin_popcount(c->what) * m;
}

// Zeroes out_dev (degree_words u64) and fills it with the degree census of
// records [0, n) of `a`, all in stream order on `s`; `cus` sizes the grid.
// The config has passed degree_config_ok for n_nrn.
hipError_t launch_degree(const SynArrays& a, uint64_t n, const abnn_degree_config& cfg, uint64_t n_nrn,
                         uint64_t* out_dev, uint32_t cus, hipStream_t s);

}  // namespace abnn
