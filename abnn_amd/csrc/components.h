// components.h -- connected components (components.hip; abnn.h
// abnn_components_*): the weakly connected components of a
// handle's records over a neuron range, a union-find in a one-u32-per-neuron
// label plane, as the C-ABI implementation (capi.hip) launches it.  The first
// half -- the config checks, the word counts and the rule on the host
// (components_host) -- includes no HIP header: g++ compiles it alone
// (tests/cpp/components_host_test.cpp).
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/abnn/abnn.h"

namespace abnn {

constexpr uint32_t kCompAllFlags = ABNN_COMP_WEIGHT | ABNN_COMP_SIZES;
constexpr uint32_t kCompNone = ABNN_COMP_NONE;
constexpr uint32_t kCompBinsAt = ABNN_COMP_HEADER_WORDS;                     // word 8
constexpr uint32_t kCompPlaneAt = ABNN_COMP_HEADER_WORDS + ABNN_COMP_SIZE_BINS;  // word 40
// word 7, the give-up codes (never set in a correct run)
constexpr uint32_t kCompGaveUpFind = 1, kCompGaveUpUnite = 2;

// The checks of abnn_components_words.
inline bool components_config_ok(const abnn_components_config* c, uint64_t n_nrn)
{
    if (!c || n_nrn == 0 || n_nrn >= (1ull << 32) || (c->flags & ~kCompAllFlags)) return false;
    if (c->count == 0 || (uint64_t)c->first + c->count > n_nrn) return false;
    for (uint32_t r : c->reserved)
        if (r != 0) return false;
    uint32_t lo, hi;
    __builtin_memcpy(&lo, &c->w_lo, 4);
    __builtin_memcpy(&hi, &c->w_hi, 4);
    if (c->flags & ABNN_COMP_WEIGHT) {
        if (!(c->w_lo < c->w_hi)) return false;  // false for a NaN bound too
    } else if (lo != 0 || hi != 0) {             // both +0.0f
        return false;
    }
    return true;
}

// u64 words of one plane (labels, sizes): N_NRN u32, an odd N_NRN padded
inline uint64_t components_plane_words(uint64_t n_nrn) { return (n_nrn + 1) / 2; }

inline uint64_t components_words(const abnn_components_config* c, uint64_t n_nrn)
{
    if (!components_config_ok(c, n_nrn)) return 0;
    return kCompPlaneAt + components_plane_words(n_nrn) * ((c->flags & ABNN_COMP_SIZES) ? 2 : 1);
}

// Is record (src, dst, w) followed?  R = [first, first + count) lies inside
// [0, N_NRN), and a tombstone's dst is 0xFFFFFFFF: a record whose dst is in R is live.
inline bool components_followed(const abnn_components_config& c, uint32_t src, uint32_t dst, float w)
{
    if (src - c.first >= c.count || dst - c.first >= c.count) return false;
    if (c.flags & ABNN_COMP_WEIGHT) return w >= c.w_lo && w < c.w_hi;  // false for NaN
    return true;
}

// Words 3..6, the bins and the size plane from a flattened label plane: the
// CLOSE step on the host.
inline void components_close_host(const abnn_components_config& c, uint64_t n_nrn, uint64_t* out)
{
    uint32_t* plane = reinterpret_cast<uint32_t*>(out + kCompPlaneAt);
    std::vector<uint32_t> size(n_nrn, 0);
    for (uint64_t n = c.first; n < (uint64_t)c.first + c.count; ++n) size[plane[n]] += 1;
    for (uint32_t j = 3; j <= 6; ++j) out[j] = 0;
    for (uint32_t j = 0; j < ABNN_COMP_SIZE_BINS; ++j) out[kCompBinsAt + j] = 0;
    for (uint64_t n = c.first; n < (uint64_t)c.first + c.count; ++n) {
        const uint32_t s = size[n];
        if (plane[n] != n) continue;  // not a label
        out[3] += 1;
        out[6] += s == 1;
        out[kCompBinsAt + (31 - __builtin_clz(s))] += 1;
        if (s > out[4]) {  // n ascends: the smallest label among equally large ones stays
            out[4] = s;
            out[5] = n;
        }
    }
    if (c.flags & ABNN_COMP_SIZES) {
        uint32_t* sizes = reinterpret_cast<uint32_t*>(out + kCompPlaneAt + components_plane_words(n_nrn));
        for (uint64_t n = 0; n < 2 * components_plane_words(n_nrn); ++n)
            sizes[n] = (n < n_nrn && (uint32_t)n - c.first < c.count) ? size[plane[n]] : 0u;
    }
}

// The rule of abnn.h over interchange records, sequentially: out holds
// components_words u64.  The config has passed components_config_ok.
inline void components_host(const abnn_components_config& c, uint64_t n_nrn, const abnn_synapse* rec, uint64_t n, uint64_t* out)
{
    for (uint64_t j = 0; j < kCompPlaneAt; ++j) out[j] = 0;
    uint32_t* plane = reinterpret_cast<uint32_t*>(out + kCompPlaneAt);
    for (uint64_t j = 0; j < 2 * components_plane_words(n_nrn); ++j)
        plane[j] = j >= n_nrn ? 0u : ((uint32_t)j - c.first < c.count ? (uint32_t)j : kCompNone);
    auto find = [&](uint32_t x) {
        while (plane[x] != x) {
            plane[x] = plane[plane[x]];  // path halving: plane[x] <= x stays
            x = plane[x];
        }
        return x;
    };
    for (uint64_t k = 0; k < n; ++k) {
        if (!components_followed(c, rec[k].src, rec[k].dst, rec[k].w)) continue;
        out[2] += 1;
        const uint32_t ru = find(rec[k].src), rv = find(rec[k].dst);
        if (ru != rv) plane[ru > rv ? ru : rv] = ru > rv ? rv : ru;  // the smaller id stays the root
    }
    for (uint64_t x = c.first; x < (uint64_t)c.first + c.count; ++x) plane[x] = find((uint32_t)x);
    out[0] = n;
    out[1] = n_nrn;
    components_close_host(c, n_nrn, out);
}

}  // namespace abnn

#if defined(__HIPCC__)
#include "engine.h"

namespace abnn {

constexpr int kCompThreads = 512;       // k_comp_link: 8 waves per workgroup
constexpr int kCompUnroll = 4;          // 16-B {dst, w} pair loads in flight per lane
constexpr int kCompPlaneThreads = 256;  // the kernels over the plane
// The settled map (components.hip): LINK unites the first kCompSlicePerNeuron x
// N_NRN records (at most half of them), flattens, and marks the neurons that
// carry the majority label of kCompSample evenly spaced neurons of R; a later
// record whose two ends are both marked is skipped.
constexpr uint64_t kCompSlicePerNeuron = 8;
constexpr uint32_t kCompSample = 1024;
// path 0 (auto) takes the settled map from this many records per neuron on
constexpr uint64_t kCompSettledMinPerNeuron = 32;

// A handle's components scratch (capi.hip allocates it as one group and frees it).
struct CompScratch {
    uint32_t* counts = nullptr;   // the size counters when SIZES is off: N_NRN u32, padded to even
    uint32_t* settled = nullptr;  // the settled map: one bit per neuron, whole u64 words
    uint32_t* major = nullptr;    // [2] the majority label of the sample
};

inline uint64_t comp_settled_words(uint64_t n_nrn) { return (n_nrn + 63) / 64 * 2; }  // u32

// One step (ABNN_COMP_BEGIN / LINK / FLATTEN / CLOSE) over records [0, n) of `a`
// in out_dev (components_words u64), in stream order on `s`.  path: 0 auto, 1
// never the settled map, 2 always.  The config has passed components_config_ok
// for n_nrn and the step is valid.
hipError_t launch_components_step(const SynArrays& a, uint64_t n, const abnn_components_config& cfg, uint64_t n_nrn,
                                  uint32_t step, uint64_t* out_dev, const CompScratch& scratch, uint32_t path, uint32_t cus,
                                  hipStream_t s);

// The shard merge: unites n with planes[p * stride + n] (stride = 2 *
// components_plane_words u32) for every n in R and p < n_planes.
hipError_t launch_components_merge(const abnn_components_config& cfg, uint64_t n_nrn, const uint32_t* planes_dev,
                                   uint32_t n_planes, uint64_t* out_dev, uint32_t cus, hipStream_t s);

}  // namespace abnn
#endif
