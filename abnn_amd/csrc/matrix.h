// matrix.h -- the population connectivity matrix (matrix.hip; abnn.h
// abnn_matrix_*): for a partition of the neurons into P
// populations, the count and the summed weight of the records from population
// a to population b for every pair, in one streaming pass, as the C-ABI
// implementation (capi.hip) launches it.  The first half -- the config checks,
// the word count and the rule on the host (matrix_host) -- includes no HIP
// header: g++ compiles it alone (tests/cpp/matrix_host_test.cpp).
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/abnn/abnn.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ABNN_MAT_HD __host__ __device__
#else
#define ABNN_MAT_HD
#endif

namespace abnn {

constexpr uint32_t kMatAllWhat = ABNN_MAT_COUNT | ABNN_MAT_W | ABNN_MAT_P;
constexpr uint32_t kMatAllFlags = ABNN_MAT_LABELS | ABNN_MAT_WEIGHT;
constexpr uint32_t kMatNone = 0xFFFFFFFFu;  // pop(n): no population
constexpr uint32_t kMatSizesAt = ABNN_MATRIX_HEADER_WORDS;

// The checks of abnn_matrix_words.
inline bool matrix_config_ok(const abnn_matrix_config* c)
{
    if (!c || c->pops < 1 || c->pops > ABNN_MATRIX_MAX_POPS) return false;
    if (c->what == 0 || (c->what & ~kMatAllWhat) || (c->flags & ~kMatAllFlags)) return false;
    for (uint32_t r : c->reserved)
        if (r != 0) return false;
    uint32_t lo, hi;
    __builtin_memcpy(&lo, &c->w_lo, 4);
    __builtin_memcpy(&hi, &c->w_hi, 4);
    if (c->flags & ABNN_MAT_WEIGHT) {
        if (!(c->w_lo < c->w_hi)) return false;  // false for a NaN bound too
    } else if (lo != 0 || hi != 0) {             // both +0.0f
        return false;
    }
    return true;
}

inline uint32_t matrix_planes(const abnn_matrix_config& c) { return (uint32_t)__builtin_popcount(c.what); }

inline uint64_t matrix_words(const abnn_matrix_config* c)
{
    if (!matrix_config_ok(c)) return 0;
    return kMatSizesAt + c->pops + (uint64_t)matrix_planes(*c) * c->pops * c->pops;
}

// bounds[0] <= ... <= bounds[P] <= n_nrn
inline bool matrix_bounds_ok(const uint32_t* bounds, uint32_t pops, uint64_t n_nrn)
{
    for (uint32_t j = 0; j < pops; ++j)
        if (bounds[j] > bounds[j + 1]) return false;
    return bounds[pops] <= n_nrn;
}

// ---- the rule, one word at a time (host and device) ---------------------------

ABNN_MAT_HD inline bool mat_weight_ok(uint32_t flags, float w, float w_lo, float w_hi)
{
    return !(flags & ABNN_MAT_WEIGHT) || (w >= w_lo && w < w_hi);  // false for NaN
}

// The fixed-point term of coefficient c (the degree census's, propagate.h
// prop_term's test), or false when c is not summable (NaN, +-inf, |c| >= 128).
ABNN_MAT_HD inline bool mat_term(float c, int32_t* q)
{
    if (!(fabsf(c) < 128.0f)) return false;
    *q = (int32_t)(c * 16777216.0f);
    return true;
}

// the P plane's coefficient: two fp32 operations (propagate.h prop_coeff with FIRE_P)
ABNN_MAT_HD inline float mat_fire_p(float w, float base_scale)
{
    const float w2 = w * w;
    return w2 * base_scale;
}

// ---- the rule on the host ------------------------------------------------------

inline uint32_t mat_pop_host(const abnn_matrix_config& c, const uint32_t* bounds, const uint32_t* labels, uint64_t n_nrn,
                             uint32_t n)
{
    if (c.flags & ABNN_MAT_LABELS) {
        if (n >= n_nrn) return kMatNone;
        return labels[n] < c.pops ? labels[n] : kMatNone;
    }
    for (uint32_t j = 0; j < c.pops; ++j)
        if (bounds[j] <= n && n < bounds[j + 1]) return j;
    return kMatNone;
}

// out holds matrix_words u64.  The config has passed matrix_config_ok, the
// bounds matrix_bounds_ok; exactly the partition the LABELS flag names is read.
inline void matrix_host(const abnn_matrix_config& c, const uint32_t* bounds, const uint32_t* labels, uint64_t n_nrn,
                        float base_scale, const abnn_synapse* rec, uint64_t n, uint64_t* out)
{
    const uint32_t P = c.pops;
    const uint64_t words = matrix_words(&c), cells = (uint64_t)P * P;
    for (uint64_t j = 0; j < words; ++j) out[j] = 0;
    uint64_t* plane = out + kMatSizesAt + P;
    uint64_t* cnt = nullptr;
    uint64_t* sw = nullptr;
    uint64_t* sp = nullptr;
    if (c.what & ABNN_MAT_COUNT) cnt = plane, plane += cells;
    if (c.what & ABNN_MAT_W) sw = plane, plane += cells;
    if (c.what & ABNN_MAT_P) sp = plane, plane += cells;
    out[0] = n;
    out[9] = P;
    out[10] = n_nrn;
    if (c.flags & ABNN_MAT_LABELS) {
        for (uint64_t x = 0; x < n_nrn; ++x)
            if (labels[x] < P) out[kMatSizesAt + labels[x]] += 1, out[11] += 1;
    } else {
        for (uint32_t j = 0; j < P; ++j) out[kMatSizesAt + j] = bounds[j + 1] - bounds[j];
        out[11] = bounds[P] - bounds[0];
    }
    for (uint64_t k = 0; k < n; ++k) {
        const abnn_synapse& r = rec[k];
        if (r.dst == 0xFFFFFFFFu) {
            out[1] += 1;
            continue;
        }
        if (!mat_weight_ok(c.flags, r.w, c.w_lo, c.w_hi)) {
            out[6] += 1;
            continue;
        }
        const uint32_t a = mat_pop_host(c, bounds, labels, n_nrn, r.src), b = mat_pop_host(c, bounds, labels, n_nrn, r.dst);
        if (a == kMatNone || b == kMatNone) {
            out[a != kMatNone ? 4 : (b != kMatNone ? 3 : 5)] += 1;
            continue;
        }
        out[2] += 1;
        const uint64_t cell = (uint64_t)a * P + b;
        int32_t q = 0;
        if (cnt) cnt[cell] += 1;
        if (sw) {
            if (mat_term(r.w, &q))
                sw[cell] += (uint64_t)(int64_t)q;
            else
                out[7] += 1;
        }
        if (sp) {
            if (mat_term(mat_fire_p(r.w, base_scale), &q))
                sp[cell] += (uint64_t)(int64_t)q;
            else
                out[8] += 1;
        }
    }
}

}  // namespace abnn

#if defined(__HIPCC__)
#include "engine.h"

namespace abnn {

constexpr int kMatThreads = 512;       // k_matrix: 8 waves per workgroup
constexpr int kMatUnroll = 4;          // 16-B {dst, w} pair loads in flight per lane
constexpr int kMatPlaneThreads = 256;  // k_matrix_pack
// a launch's accumulators fit this; W | P of 64 populations and COUNT | W | P of
// more than 57 do not and are scanned twice (the planes asked without P, then P)
constexpr uint32_t kMatLdsBytes = 64 * 1024;

// abnn_debug_set_matrix_path: how a record's cell is added (RUNS: scan.h / runs.h
// run aggregation, a wave in one cell adds once; ATOMIC: one LDS atomic per
// record and plane) and where a LABELS scan reads a neuron's population (PACKED:
// the handle's one-byte-per-neuron copy; DIRECT: the caller's u32 plane).
constexpr uint32_t kMatPathAuto = 0, kMatPathRunsPacked = 1, kMatPathRunsDirect = 2, kMatPathAtomicPacked = 3,
                   kMatPathAtomicDirect = 4;

// Zeroes out_dev (matrix_words u64) and fills it with the matrix of records
// [0, n) of `a`, all in stream order on `s`; `cus` sizes the grid.  The config
// and the bounds have passed their checks; bounds is host memory (read before
// the call returns), labels_dev device memory, pack_dev the handle's N_NRN
// bytes (LABELS only).
hipError_t launch_matrix(const SynArrays& a, uint64_t n, const abnn_matrix_config& cfg, const uint32_t* bounds,
                         const uint32_t* labels_dev, uint64_t n_nrn, float base_scale, uint8_t* pack_dev, uint32_t path,
                         uint64_t* out_dev, uint32_t cus, hipStream_t s);

}  // namespace abnn
#endif
