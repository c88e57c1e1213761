// snapshot.h -- device-side snapshots (snapshot.hip; abnn.h abnn_snapshot_*,
// DESIGN.md §9).  Capture and restore are device-to-device copies plus the
// handle's bookkeeping (capi.hip); the diff is one streaming pass over two
// record arrays.  The diff's rule lives here ONCE, as __host__ __device__
// inlines: the kernel (snapshot.hip k_diff) and abnn_snapshot_diff_host
// (capi.hip) both call diff_record, so they cannot drift apart.  The rule's part
// of this header needs nothing but abnn.h, so a plain C++ compiler can build it
// (tests/cpp/snapshot_host_test.cpp).
#pragma once

#include <cstdint>

#include "../../include/abnn/abnn.h"

#if defined(__HIPCC__)
#define ABNN_SNAP_HD __host__ __device__
#else
#define ABNN_SNAP_HD
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace abnn {

constexpr uint32_t kDiffTomb = 0xFFFFFFFFu;   // the tombstone's dst
constexpr uint32_t kDiffNoBin = 0xFFFFFFFFu;  // diff_record: the record goes to no bin

ABNN_SNAP_HD inline uint32_t diff_bits(float x)
{
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    return u;
}

ABNN_SNAP_HD inline float diff_float(uint32_t u)
{
    float x;
    __builtin_memcpy(&x, &u, 4);
    return x;
}

inline bool diff_finite(float x) { return (diff_bits(x) & 0x7F800000u) != 0x7F800000u; }

// The checks of abnn_snapshot_diff_words (abnn_census_words' over the same
// fields); *scale = (float)bins / (hi - lo), one fp32 division.
inline bool diff_config_ok(const abnn_diff_config* c, float* scale)
{
    if (!c || c->bins < 1 || c->bins > ABNN_DIFF_MAX_BINS || c->reserved != 0) return false;
    if (!diff_finite(c->lo) || !diff_finite(c->hi) || !(c->lo < c->hi)) return false;
    const volatile float span = c->hi - c->lo;  // volatile: a single rounded fp32 operation each
    const volatile float s = (float)c->bins / span;
    if (!diff_finite(span) || !diff_finite(s)) return false;
    if (scale) *scale = s;
    return true;
}

inline uint64_t diff_words(const abnn_diff_config* c)
{
    return diff_config_ok(c, nullptr) ? ABNN_DIFF_HEADER_WORDS + (uint64_t)c->bins : 0;
}

// A config that passed diff_config_ok, as the rule reads it.
struct DiffRule {
    float lo, hi, scale;
    uint32_t bins;
    uint32_t src_first, src_count, dst_first, dst_count;  // count 0: any
};

inline DiffRule diff_rule(const abnn_diff_config& c, float scale)
{
    return DiffRule{c.lo, c.hi, scale, c.bins, c.src_first, c.src_count, c.dst_first, c.dst_count};
}

// Result words 5 .. 18 and 21 (counts), 19 / 20 (net / abs) and 22 (the
// maximum); C is u32 in a kernel thread, u64 on the host.
template <typename C>
struct DiffTally {
    C count[14] = {};  // word 5 + j
    C not_summable = 0;
    int64_t net = 0;
    uint64_t abs = 0;
    uint32_t max_bits = 0;
};
enum : uint32_t {
    kDiffDeadBoth = 0, kDiffKilled, kDiffRevived, kDiffRewired, kDiffPaired, kDiffSelected, kDiffSame, kDiffChanged,
    kDiffUp, kDiffDown, kDiffZero, kDiffNan, kDiffUnder, kDiffOver
};

// One record pair: A = {sa, da, wa} of `then`, B of `now` (src, dst, weight
// bits).  Counts it and returns its bin, or kDiffNoBin.
template <typename C>
ABNN_SNAP_HD inline uint32_t diff_record(const DiffRule& r, uint32_t sa, uint32_t da, uint32_t wa, uint32_t sb,
                                         uint32_t db, uint32_t wb, DiffTally<C>& t)
{
    const bool ta = da == kDiffTomb, tb = db == kDiffTomb;
    if (ta || tb) {
        // constant indices: the kernel keeps the counts in registers
        t.count[kDiffDeadBoth] += ta && tb ? 1 : 0;
        t.count[kDiffKilled] += !ta ? 1 : 0;
        t.count[kDiffRevived] += !tb ? 1 : 0;
        return kDiffNoBin;
    }
    if (sa != sb || da != db) {
        t.count[kDiffRewired] += 1;
        return kDiffNoBin;
    }
    t.count[kDiffPaired] += 1;
    if (r.src_count && !(sb - r.src_first < r.src_count)) return kDiffNoBin;
    if (r.dst_count && !(db - r.dst_first < r.dst_count)) return kDiffNoBin;
    t.count[kDiffSelected] += 1;
    if (wa == wb) {
        t.count[kDiffSame] += 1;
        return kDiffNoBin;
    }
    t.count[kDiffChanged] += 1;
    // the fixed-point sums: |w| < 128 on the bits (false for NaN and +-inf)
    if ((wa & 0x7FFFFFFFu) < 0x43000000u && (wb & 0x7FFFFFFFu) < 0x43000000u) {
        const float pa = diff_float(wa) * 16777216.0f, pb = diff_float(wb) * 16777216.0f;
        const int64_t q = (int64_t)(int32_t)pb - (int64_t)(int32_t)pa;
        t.net = (int64_t)((uint64_t)t.net + (uint64_t)q);
        t.abs += (uint64_t)(q < 0 ? -q : q);
    } else {
        t.not_summable += 1;
    }
    const float d = diff_float(wb) - diff_float(wa);
    if (d != d) {
        t.count[kDiffNan] += 1;
        return kDiffNoBin;
    }
    t.count[kDiffUp] += d > 0.0f ? 1 : 0;
    t.count[kDiffDown] += d < 0.0f ? 1 : 0;
    t.count[kDiffZero] += d == 0.0f ? 1 : 0;
    const uint32_t ad = diff_bits(d) & 0x7FFFFFFFu;
    t.max_bits = ad > t.max_bits ? ad : t.max_bits;
    if (d < r.lo) {
        t.count[kDiffUnder] += 1;
        return kDiffNoBin;
    }
    if (d >= r.hi) {
        t.count[kDiffOver] += 1;
        return kDiffNoBin;
    }
    const float x = d - r.lo;
    const float y = x * r.scale;
    const uint32_t bin = (uint32_t)y;
    return bin < r.bins - 1 ? bin : r.bins - 1;
}

// The rule over interchange records (abnn_snapshot_diff_host): the config has
// passed diff_config_ok, out holds diff_words(&c) u64.
inline void diff_host(const abnn_diff_config& c, float scale, const abnn_synapse* then, uint64_t n_then,
                      const abnn_synapse* now, uint64_t n_now, uint64_t* out)
{
    const DiffRule r = diff_rule(c, scale);
    const uint64_t cmp = n_then < n_now ? n_then : n_now;
    for (uint64_t i = 0; i < ABNN_DIFF_HEADER_WORDS + (uint64_t)c.bins; ++i) out[i] = 0;
    DiffTally<uint64_t> t;
    for (uint64_t k = 0; k < cmp; ++k) {
        const uint32_t bin = diff_record(r, then[k].src, then[k].dst, diff_bits(then[k].w), now[k].src, now[k].dst,
                                         diff_bits(now[k].w), t);
        if (bin != kDiffNoBin) out[ABNN_DIFF_HEADER_WORDS + bin] += 1;
    }
    out[0] = n_now;
    out[1] = n_then;
    out[2] = cmp;
    out[3] = n_now - cmp;
    out[4] = n_then - cmp;
    for (uint32_t j = 0; j < 14; ++j) out[5 + j] = t.count[j];
    out[19] = (uint64_t)t.net;
    out[20] = t.abs;
    out[21] = t.not_summable;
    out[22] = t.max_bits;
}

}  // namespace abnn

#if defined(__HIPCC__)
#include "engine.h"

namespace abnn {

constexpr int kDiffThreads = 512;  // 8 waves per workgroup
// 16-B loads in flight per lane and side.  Measured at config 3: 2 -> 3.55 ms (80 VGPRs, three workgroups per
// CU), 1 -> 3.80 ms, 4 -> 5.33 ms (144 VGPRs leave one workgroup per CU)
constexpr int kDiffUnroll = 2;

// Zeroes out_dev (diff_words u64) and fills it with the diff of records
// [0, min(n_then, n_now)) of `then` and `now` (lo, hi and dw; src32 is not
// read), all in stream order on `s`; `cus` sizes the grid.  Nothing at or past
// the shorter side's end is read.
hipError_t launch_diff(const SynArrays& then, uint64_t n_then, const SynArrays& now, uint64_t n_now,
                       const DiffRule& rule, uint64_t* out_dev, uint32_t cus, hipStream_t s);
// src32[i] = the src the two streams hold, records [0, n): the random-mode
// mirror brought back in step after the streams were copied over.
hipError_t launch_src32_sync(const SynArrays& a, uint64_t n, hipStream_t s);

}  // namespace abnn
#endif
