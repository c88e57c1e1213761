// census.h -- the synapse census (census.hip; abnn.h abnn_census_*, DESIGN.md
// §9): one streaming pass over a handle's records that counts tombstones and
// bins the selected weights, as the C-ABI implementation (capi.hip) launches it.
#pragma once

#include <cmath>

#include "engine.h"

namespace abnn {

constexpr int kCensusThreads = 512;          // 8 waves per workgroup
constexpr int kCensusUnroll = 4;             // 16-B loads in flight per lane

// The checks of abnn_census_words (everything that needs no handle); *scale =
// (float)bins / (hi - lo), one fp32 division.
inline bool census_config_ok(const abnn_census_config* c, float* scale)
{
    if (!c || c->bins < 1 || c->bins > ABNN_CENSUS_MAX_BINS || c->reserved != 0) return false;
    if (!std::isfinite(c->lo) || !std::isfinite(c->hi) || !(c->lo < c->hi)) return false;
    const volatile float span = c->hi - c->lo;  // volatile: a single rounded fp32 operation each
    const volatile float s = (float)c->bins / span;
    if (!std::isfinite(span) || !std::isfinite(s)) return false;
    if (scale) *scale = s;
    return true;
}

// Zeroes out_dev (ABNN_CENSUS_HEADER_WORDS + bins u64) and fills it with the
// census of records [0, n) of `a`, all in stream order on `s`; `cus` sizes the
// grid.  The config has passed census_config_ok and the range checks.
hipError_t launch_census(const SynArrays& a, uint64_t n, const abnn_census_config& cfg, float scale,
                         uint64_t* out_dev, uint32_t cus, hipStream_t s);

}  // namespace abnn
