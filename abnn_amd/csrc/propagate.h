// propagate.h -- signal propagation (propagate.hip; abnn.h abnn_propagate_*,
// DESIGN.md §9): the handle's records used as the sparse matrix they are, one
// streaming pass y[kout] += c(w) * x[kin] in integers, the rescale of y into the
// next x and the iteration of both, as the C-ABI implementation (capi.hip)
// launches them; and the same rule on the host (abnn_propagate_host), written
// once for both.
#pragma once

#include <cmath>

#include "engine.h"

namespace abnn {

constexpr int kPropThreads = 512;     // k_propagate: 8 waves per workgroup
constexpr int kPropFwdUnroll = 2;     // sparse forward: 16-B lo + 8-B hi loads (8 records each) in flight per lane
constexpr int kPropPairUnroll = 4;    // dense and reverse: 16-B {dst, w} pair loads in flight per lane
constexpr int kPropPlaneThreads = 256;  // k_prop_map / k_prop_reduce / k_prop_rescale
// Out-ranges of at most this many neurons accumulate in LDS (narrow), longer
// ones by atomics into the result (wide).  Mirrored by abnn_amd/propagate.py NARROW_MAX.
constexpr uint32_t kPropNarrowMax = 4096;
// Forward, the sparse instance runs when nnz * kPropSparseDiv <= N_NRN (nnz: the
// non-zero x of the in-range, counted on the device), the dense one otherwise.
// Measured at config 3 (tools/propagate_bench.py): the sparse
// instance is the faster one down to one non-zero neuron in four (the dense one
// gathers x[src] for every record); the first version had 64 here.
// Mirrored by abnn_amd/propagate.py SPARSE_DIV.
constexpr uint32_t kPropSparseDiv = 4;
// The sparse instance folds the non-zero map to this many u32 words in LDS
// (16 KiB, beside a narrow out-range's 32 KiB) when nnz is at most
// kPropFoldMaxNnz (at most every second folded bit is then set: a record whose
// bit is clear is rejected from LDS, one that passes is confirmed against the
// map in the L2) or when the whole map fits.  Mirrored by abnn_amd/propagate.py
// FOLD_WORDS / FOLD_MAX_NNZ.
constexpr uint32_t kPropFoldWords = 4096;
constexpr uint32_t kPropFoldMaxNnz = 32 * kPropFoldWords / 2;
constexpr uint32_t kPropMaxSteps = 4096;  // abnn_propagate_iterate_enqueue

constexpr uint32_t kPropAllFlags = ABNN_PROP_REVERSE | ABNN_PROP_FIRE_P | ABNN_PROP_WEIGHT;

// The checks of abnn_propagate_words; *m_out = the neurons of the out-range.
inline bool propagate_config_ok(const abnn_propagate_config* c, uint64_t n_nrn, uint64_t* m_out)
{
    if (!c || n_nrn == 0 || n_nrn > 0xFFFFFFFFull || (c->flags & ~kPropAllFlags)) return false;  // neuron ids are u32
    for (uint32_t r : c->reserved)
        if (r != 0) return false;
    if (c->in_count == 0 && c->in_first != 0) return false;
    if (c->out_count == 0 && c->out_first != 0) return false;
    if ((uint64_t)c->in_first + c->in_count > n_nrn || (uint64_t)c->out_first + c->out_count > n_nrn) return false;
    uint32_t lo, hi;
    __builtin_memcpy(&lo, &c->w_lo, 4);
    __builtin_memcpy(&hi, &c->w_hi, 4);
    if (c->flags & ABNN_PROP_WEIGHT) {
        if (!(c->w_lo < c->w_hi)) return false;  // false for a NaN bound too
    } else if (lo != 0 || hi != 0) {             // both +0.0f
        return false;
    }
    if (m_out) *m_out = c->out_count ? (uint64_t)c->out_count : n_nrn;
    return true;
}

inline uint64_t propagate_words(const abnn_propagate_config* c, uint64_t n_nrn)
{
    uint64_t m = 0;
    if (!propagate_config_ok(c, n_nrn, &m)) return 0;
    return ABNN_PROP_HEADER_WORDS + m;
}

// iterate: the next x is the rescaled y, so both ranges are one
inline bool propagate_ranges_equal(const abnn_propagate_config& c)
{
    return c.in_first == c.out_first && c.in_count == c.out_count;
}

// A config's ranges with count 0 resolved to every neuron.
struct PropRanges {
    uint32_t in_first, in_count, out_first, out_count;
};

inline PropRanges propagate_ranges(const abnn_propagate_config& c, uint64_t n_nrn)
{
    return PropRanges{c.in_count ? c.in_first : 0u, c.in_count ? c.in_count : (uint32_t)n_nrn,
                      c.out_count ? c.out_first : 0u, c.out_count ? c.out_count : (uint32_t)n_nrn};
}

// ---- the rule, one word at a time (host and device) ---------------------------

__host__ __device__ inline bool prop_weight_ok(uint32_t flags, float w, float w_lo, float w_hi)
{
    return !(flags & ABNN_PROP_WEIGHT) || (w >= w_lo && w < w_hi);  // false for NaN
}

// c(w): w, or with FIRE_P the fire probability (w*w)*base_scale, two fp32
// operations in the reference's order (no contraction: there is no add)
__host__ __device__ inline float prop_coeff(uint32_t flags, float w, float base_scale)
{
    if (!(flags & ABNN_PROP_FIRE_P)) return w;
    const float w2 = w * w;
    return w2 * base_scale;
}

// The term of a followed record, or false when c is not summable (NaN, +-inf,
// |c| >= 128).  q is the degree census's term; the shift is arithmetic (a floor).
__host__ __device__ inline bool prop_term(float c, int32_t x, int64_t* term)
{
    if (!(fabsf(c) < 128.0f)) return false;
    const int32_t q = (int32_t)(c * 16777216.0f);
    *term = ((int64_t)q * (int64_t)x) >> 16;
    return true;
}

__host__ __device__ inline uint64_t prop_abs32(int32_t v) { return v < 0 ? (uint64_t)(-(int64_t)v) : (uint64_t)v; }
// |y| as u64: INT64_MIN counts as 2^63
__host__ __device__ inline uint64_t prop_abs64(uint64_t y) { return (int64_t)y < 0 ? 0ull - y : y; }

// The rescale's exponent for the largest magnitude Mx: 30 - bit length, 0 for Mx == 0.
__host__ __device__ inline int32_t prop_exponent(uint64_t mx)
{
    if (mx == 0) return 0;
    return 30 - (64 - (int32_t)__builtin_clzll(mx));
}

// y scaled by 2^e (a right shift is arithmetic), truncated to 32 bits.
__host__ __device__ inline int32_t prop_rescaled(uint64_t y, int32_t e)
{
    const uint64_t r = e >= 0 ? y << e : (uint64_t)((int64_t)y >> -e);
    return (int32_t)(uint32_t)r;
}

// ---- the rule on the host ------------------------------------------------------

// out holds propagate_words u64; x holds n_nrn values.  The config has passed
// propagate_config_ok for n_nrn.
inline void propagate_host(const abnn_propagate_config& c, uint64_t n_nrn, float base_scale, const abnn_synapse* syn,
                           uint64_t n, const int32_t* x, uint64_t* out)
{
    const PropRanges r = propagate_ranges(c, n_nrn);
    for (uint64_t j = 0; j < ABNN_PROP_HEADER_WORDS + (uint64_t)r.out_count; ++j) out[j] = 0;
    uint64_t* y = out + ABNN_PROP_HEADER_WORDS;
    out[0] = n;
    for (uint32_t j = 0; j < r.in_count; ++j) {
        const int32_t v = x[r.in_first + j];
        out[4] += v != 0;
        out[5] += prop_abs32(v);
    }
    const bool rev = c.flags & ABNN_PROP_REVERSE;
    for (uint64_t i = 0; i < n; ++i) {
        const abnn_synapse& s = syn[i];
        if (s.dst == 0xFFFFFFFFu) {
            out[1] += 1;
            continue;
        }
        const uint32_t kin = rev ? s.dst : s.src, kout = rev ? s.src : s.dst;
        if (kin - r.in_first >= r.in_count || kout - r.out_first >= r.out_count) continue;
        if (!prop_weight_ok(c.flags, s.w, c.w_lo, c.w_hi)) continue;
        const int32_t xv = x[kin];
        if (xv == 0) continue;
        out[2] += 1;
        int64_t term = 0;
        if (!prop_term(prop_coeff(c.flags, s.w, base_scale), xv, &term)) {
            out[3] += 1;
            continue;
        }
        y[kout - r.out_first] += (uint64_t)term;
    }
}

// The rescale of a result `out` into x over the out-range; row holds 8 u64.
inline void propagate_rescale_host(const abnn_propagate_config& c, uint64_t n_nrn, const uint64_t* out, int32_t* x,
                                   uint64_t* row)
{
    const PropRanges r = propagate_ranges(c, n_nrn);
    const uint64_t* y = out + ABNN_PROP_HEADER_WORDS;
    uint64_t sum = 0, mx = 0;
    for (uint32_t j = 0; j < r.out_count; ++j) {
        const uint64_t a = prop_abs64(y[j]);
        sum += a;
        mx = a > mx ? a : mx;
    }
    const int32_t e = prop_exponent(mx);
    for (uint32_t j = 0; j < r.out_count; ++j) x[r.out_first + j] = prop_rescaled(y[j], e);
    if (row) {
        const uint64_t w[8] = {out[4], out[5], sum, mx, (uint64_t)(int64_t)e, out[2], out[3], 0};
        for (int j = 0; j < 8; ++j) row[j] = w[j];
    }
}

// ---- the device launches (propagate.hip) ----------------------------------------

// The scratch of a handle's propagations (owned by its DevicePool).
struct PropScratch {
    uint32_t* map = nullptr;   // one bit per neuron: x != 0 inside the in-range; every word written by k_prop_map
    uint64_t* red = nullptr;   // the rescale's reduce words: sum |y|, max |y|
};

// Zeroes out_dev (propagate_words u64) and fills it with the propagation of
// x_dev (n_nrn int32, 16-byte aligned) over records [0, n) of `a`, all in
// stream order on `s`; `path` 0 = the device chooses the forward instance, 1 =
// sparse, 2 = dense; `cus` sizes the grids.  The config has passed
// propagate_config_ok for n_nrn.
hipError_t launch_propagate(const SynArrays& a, uint64_t n, const abnn_propagate_config& cfg, uint64_t n_nrn, float base_scale,
                            const int32_t* x_dev, uint64_t* out_dev, const PropScratch& scratch, uint32_t path,
                            uint32_t cus, hipStream_t s);

// The rescale of out_dev into x_dev over the out-range and, when row_dev is
// not null, its trace row (8 u64), in stream order on `s`.
hipError_t launch_propagate_rescale(const abnn_propagate_config& cfg, uint64_t n_nrn, const uint64_t* out_dev, int32_t* x_dev,
                                    uint64_t* row_dev, const PropScratch& scratch, uint32_t cus, hipStream_t s);

}  // namespace abnn
