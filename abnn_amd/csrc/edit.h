// edit.h -- the synapse edit (edit.hip; abnn.h abnn_edit_*): one
// streaming read-modify-write pass over a handle's records.  The rule lives
// here ONCE, as __host__ __device__ inlines: the kernel (edit.hip k_edit) and
// abnn_edit_host (capi.hip) both call edit_match / edit_value / edit_factor, so
// they cannot drift apart.  The rule's part of this header needs nothing but
// abnn.h, so a plain C++ compiler can build it (tests/cpp/edit_host_test.cpp).
#pragma once

#include <cstdint>

#include "../../include/abnn/abnn.h"

#if defined(__HIPCC__)
#define ABNN_EDIT_HD __host__ __device__
#else
#define ABNN_EDIT_HD
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace abnn {

constexpr uint32_t kEditAllFlags = ABNN_EDIT_ANY | ABNN_EDIT_WEIGHT | ABNN_EDIT_CLAMP;
constexpr uint32_t kEditOps = 6;
constexpr uint32_t kEditTomb = 0xFFFFFFFFu;  // the tombstone's dst (and interchange src)
constexpr uint32_t kEditNaN = 0x7FC00000u;   // the NaN an edit stores (abnn.h)

ABNN_EDIT_HD inline uint32_t edit_bits(float x)
{
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    return u;
}

ABNN_EDIT_HD inline float edit_float(uint32_t u)
{
    float x;
    __builtin_memcpy(&x, &u, 4);
    return x;
}

ABNN_EDIT_HD inline bool edit_is_scale(uint32_t op) { return op == ABNN_EDIT_SCALE_DST || op == ABNN_EDIT_SCALE_SRC; }
ABNN_EDIT_HD inline bool edit_nonfinite(uint32_t bits) { return (bits & 0x7F800000u) == 0x7F800000u; }  // NaN, +-inf

// The checks of abnn_edit_words (everything that needs no handle).
inline bool edit_config_ok(const abnn_edit_config* c)
{
    if (!c || (c->flags & ~kEditAllFlags) || c->op >= kEditOps) return false;
    if (c->reserved[0] != 0 || c->reserved[1] != 0) return false;
    // the shared fields: abnn_select_words' checks (select.h select_config_ok)
    if ((uint64_t)c->src_first + c->src_count > (1ull << 32)) return false;
    if ((uint64_t)c->dst_first + c->dst_count > (1ull << 32)) return false;
    if ((c->flags & ABNN_EDIT_ANY) && c->src_count == 0 && c->dst_count == 0) return false;
    if (c->flags & ABNN_EDIT_WEIGHT) {
        if (!(c->w_lo < c->w_hi)) return false;  // false for a NaN bound too
    } else if (edit_bits(c->w_lo) != 0 || edit_bits(c->w_hi) != 0) {
        return false;
    }
    const uint32_t op = c->op;
    const bool clamp = (c->flags & ABNN_EDIT_CLAMP) != 0;
    const bool reads_a = op == ABNN_EDIT_AFFINE || op == ABNN_EDIT_DRAW;
    const bool reads_b = reads_a || op == ABNN_EDIT_SET;
    if (reads_a ? c->a != c->a : edit_bits(c->a) != 0) return false;  // a NaN where read, any bit where not
    if (reads_b ? c->b != c->b : edit_bits(c->b) != 0) return false;
    if (clamp) {
        if (op == ABNN_EDIT_KILL) return false;
        if (!(c->c_lo <= c->c_hi)) return false;  // false for a NaN bound too
    } else if (edit_bits(c->c_lo) != 0 || edit_bits(c->c_hi) != 0) {
        return false;
    }
    if (op == ABNN_EDIT_DRAW) {
        const float inf = __builtin_inff();
        if (!(c->a > -inf && c->a < inf && c->b > -inf && c->b < inf)) return false;
        if (!(c->a <= c->b)) return false;
    } else if (c->seed != 0) {
        return false;
    }
    if ((c->flags & ABNN_EDIT_ANY) && edit_is_scale(op)) return false;
    return true;
}

inline uint64_t edit_words(const abnn_edit_config* c) { return edit_config_ok(c) ? ABNN_EDIT_HEADER_WORDS : 0; }

// A config as the per-record functions take it (by value in the kernel's
// arguments).  Ranges as {first, span}, select.hip's: x is inside iff x - first
// < span; a range that is not set has span 0xFFFFFFFF (every live value passes)
// without ANY and span 0 (none does) with it.
struct EditRule {
    uint32_t src_first, src_span, dst_first, dst_span;
    uint32_t any, weight, op, clamp;
    float w_lo, w_hi, a, b, c_lo, c_hi;
    uint32_t plane_first, plane_count;  // SCALE: the plane holds keys [first, first + count)
    uint64_t key;                       // DRAW: seed ^ ABNN_EDIT_KEY
    uint64_t syn_offset;
};

// of a config that passed edit_config_ok; the ranges end at or below n_nrn
inline EditRule edit_rule(const abnn_edit_config& c, uint64_t n_nrn, uint64_t syn_offset)
{
    EditRule r;
    __builtin_memset(&r, 0, sizeof(r));
    r.any = (c.flags & ABNN_EDIT_ANY) ? 1u : 0u;
    r.weight = (c.flags & ABNN_EDIT_WEIGHT) ? 1u : 0u;
    r.clamp = (c.flags & ABNN_EDIT_CLAMP) ? 1u : 0u;
    r.op = c.op;
    const uint32_t unset = r.any ? 0u : 0xFFFFFFFFu;
    r.src_first = c.src_count ? c.src_first : 0u;
    r.src_span = c.src_count ? c.src_count : unset;
    r.dst_first = c.dst_count ? c.dst_first : 0u;
    r.dst_span = c.dst_count ? c.dst_count : unset;
    r.w_lo = c.w_lo;
    r.w_hi = c.w_hi;
    r.a = c.a;
    r.b = c.b;
    r.c_lo = c.c_lo;
    r.c_hi = c.c_hi;
    if (edit_is_scale(c.op)) {
        const bool dst = c.op == ABNN_EDIT_SCALE_DST;
        const uint32_t first = dst ? c.dst_first : c.src_first, count = dst ? c.dst_count : c.src_count;
        r.plane_first = count ? first : 0u;
        r.plane_count = count ? count : (uint32_t)n_nrn;
    }
    r.key = c.seed ^ ABNN_EDIT_KEY;
    r.syn_offset = syn_offset;
    return r;
}

// The entries of a SCALE op's plane (M), 0 for another op.
inline uint64_t edit_plane_count(const abnn_edit_config& c, uint64_t n_nrn)
{
    if (!edit_is_scale(c.op)) return 0;
    const uint32_t count = c.op == ABNN_EDIT_SCALE_DST ? c.dst_count : c.src_count;
    return count ? count : n_nrn;
}

// abnn_select's matching rule (select.hip match).  kSrc = false: the caller
// knows that no src range is set and passes any src.
template <bool kSrc = true>
ABNN_EDIT_HD inline bool edit_match(const EditRule& r, uint32_t src, uint32_t dst, uint32_t wbits)
{
    if (dst == kEditTomb) return false;
    const bool D = dst - r.dst_first < r.dst_span;
    const bool S = kSrc ? src - r.src_first < r.src_span : r.any == 0;
    bool m = r.any ? (S || D) : (S && D);
    if (r.weight) {
        const float w = edit_float(wbits);
        m = m && w >= r.w_lo && w < r.w_hi;  // false for NaN
    }
    return m;
}

// splitmix64_at and unit24 of the graph builder (graph.h)
ABNN_EDIT_HD inline uint64_t edit_splitmix64_at(uint64_t seed, uint64_t k)
{
    uint64_t z = seed + (k + 1u) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The key of a matched record into a SCALE op's plane; edit_has_factor: it lies inside.
ABNN_EDIT_HD inline uint32_t edit_plane_index(const EditRule& r, uint32_t src, uint32_t dst)
{
    return (r.op == ABNN_EDIT_SCALE_DST ? dst : src) - r.plane_first;
}

// The bits stored for a matched record of any op but KILL: `factor` is
// plane[edit_plane_index] (SCALE, read only then), i the local index (DRAW).
ABNN_EDIT_HD inline uint32_t edit_value(const EditRule& r, uint32_t wbits, float factor, uint64_t i)
{
    const float w = edit_float(wbits);
    float v;
    if (r.op == ABNN_EDIT_SET) {
        v = r.b;
    } else if (r.op == ABNN_EDIT_AFFINE) {
        const float t = w * r.a;
        v = t + r.b;
    } else if (r.op == ABNN_EDIT_DRAW) {
        const float u = (float)(edit_splitmix64_at(r.key, r.syn_offset + i) >> 40) * (1.0f / 16777216.0f);  // unit24
        const float d = r.b - r.a;
        const float t = u * d;
        v = r.a + t;
    } else {  // SCALE_DST / SCALE_SRC
        v = w * factor;
    }
    if (r.clamp) {
        if (v < r.c_lo) v = r.c_lo;
        if (v > r.c_hi) v = r.c_hi;
    }
    // IEEE leaves a NaN's sign and payload open (inf * 0 is 0x7FC00000 on the
    // device, 0xFFC00000 on an x86 host): every NaN is stored as the one below
    return v != v ? kEditNaN : edit_bits(v);
}

// abnn_edit_factors_*: one factor from one strength word.
ABNN_EDIT_HD inline float edit_factor(uint64_t word, float target, float f_lo, float f_hi)
{
    const float c = (float)(int64_t)word;  // round to nearest even
    const float S = c * (1.0f / 16777216.0f);
    float f = S > 0.0f ? target / S : 1.0f;
    if (f < f_lo) f = f_lo;
    if (f > f_hi) f = f_hi;
    return f;
}

inline bool edit_factors_ok(float target, float f_lo, float f_hi)
{
    const float inf = __builtin_inff();
    return target > 0.0f && target < inf && f_lo > 0.0f && f_lo <= f_hi && f_hi < inf;
}

// The rule over n interchange records in place (abnn_edit_host): the config has
// passed edit_config_ok and the range checks, plane holds edit_plane_count
// entries for a SCALE op.
inline void edit_host(const abnn_edit_config& c, uint64_t n_nrn, uint64_t syn_offset, abnn_synapse* rec, uint64_t n,
                      const float* plane, uint64_t out[ABNN_EDIT_HEADER_WORDS])
{
    const EditRule r = edit_rule(c, n_nrn, syn_offset);
    uint64_t tomb = 0, matched = 0, changed = 0, killed = 0, bad = 0;
    for (uint64_t i = 0; i < n; ++i) {
        abnn_synapse& s = rec[i];
        tomb += s.dst == kEditTomb;
        const uint32_t old = edit_bits(s.w);
        if (!edit_match<true>(r, s.src, s.dst, old)) continue;
        ++matched;
        if (r.op == ABNN_EDIT_KILL) {
            s.src = s.dst = kEditTomb;
            s.pad = 0.0f;
            ++killed;
            ++changed;  // no v is stored: word 5 counts nothing
            continue;
        }
        uint32_t v = old;
        if (edit_is_scale(r.op)) {
            const uint32_t k = edit_plane_index(r, s.src, s.dst);
            if (k < r.plane_count) v = edit_value(r, old, plane[k], i);
        } else {
            v = edit_value(r, old, 0.0f, i);
        }
        changed += v != old;
        bad += edit_nonfinite(v);
        s.w = edit_float(v);
    }
    out[0] = n;
    out[1] = tomb;
    out[2] = matched;
    out[3] = changed;
    out[4] = killed;
    out[5] = bad;
    out[6] = out[7] = 0;
}

inline void edit_factors_host(const uint64_t* strength, uint64_t count, float target, float f_lo, float f_hi, float* plane)
{
    for (uint64_t i = 0; i < count; ++i) plane[i] = edit_factor(strength[i], target, f_lo, f_hi);
}

}  // namespace abnn

#if defined(__HIPCC__)
#include "engine.h"

namespace abnn {

// Zeroes the 8 header words of out_dev and edits records [0, n) of `a` by the
// rule (a config that passed edit_config_ok and the range checks), all in
// stream order on `s`: one persistent grid-stride launch of at most `blocks`
// workgroups.  dead: the structural update's tally, or null.  nt: non-temporal
// stores.  Nothing at or past n is read or written.
hipError_t launch_edit(const SynArrays& a, uint64_t n, const EditRule& rule, const float* plane_dev, uint32_t* dead,
                       uint64_t* out_dev, uint32_t blocks, bool nt, hipStream_t s);
hipError_t launch_edit_factors(const uint64_t* strength_dev, uint64_t count, float target, float f_lo, float f_hi,
                               float* plane_dev, uint32_t blocks, hipStream_t s);

}  // namespace abnn
#endif
