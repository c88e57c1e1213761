// corr.h -- spike correlograms (corr.hip; abnn.h abnn_corr_*):
// lag histograms of the recorder's raster over a window of table rows, for two
// populations (POP), per pair of neurons (PAIRS) or over the followed records
// (SYNAPSES).  The rule lives here ONCE, as __host__ __device__ inlines: the
// kernels (corr.hip) and abnn_corr_host (capi.hip) share the config checks, the
// window, the row clamp, the population test, the followed-record test and the
// lag bin, so they cannot drift apart.  The rule's part of this header needs
// nothing but abnn.h, so a plain C++ compiler can build it
// (tests/cpp/corr_host_test.cpp).
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/abnn/abnn.h"

#if defined(__HIPCC__)
#define ABNN_CORR_HD __host__ __device__
#else
#define ABNN_CORR_HD
#endif

namespace abnn {

constexpr uint32_t kCorrTomb = 0xFFFFFFFFu;  // the tombstone's dst

// The checks of abnn_corr_words; *plane = the plane's u64 words.
inline bool corr_config_ok(const abnn_corr_config* c, uint64_t* plane)
{
    if (!c || c->mode > ABNN_CORR_SYNAPSES || (c->flags & ~ABNN_CORR_WEIGHT) || c->max_lag > ABNN_CORR_MAX_LAG) return false;
    for (uint32_t r : c->reserved)
        if (r != 0) return false;
    if ((uint64_t)c->a_first + c->a_count > (1ull << 32)) return false;  // a range that wraps u32
    if ((uint64_t)c->b_first + c->b_count > (1ull << 32)) return false;
    uint32_t lo, hi;
    __builtin_memcpy(&lo, &c->w_lo, 4);
    __builtin_memcpy(&hi, &c->w_hi, 4);
    if (c->flags & ABNN_CORR_WEIGHT) {
        if (!(c->w_lo < c->w_hi)) return false;  // false for a NaN bound too
    } else if (lo != 0 || hi != 0) {             // both +0.0f
        return false;
    }
    uint64_t words = 2ull * c->max_lag + 1;
    if (c->mode == ABNN_CORR_PAIRS) {
        if (c->a_count == 0 || c->b_count == 0) return false;
        const uint64_t cells = (uint64_t)c->a_count * c->b_count;  // < 2^64
        if (cells > ABNN_CORR_MAX_PAIR_WORDS / words) return false;
        words *= cells;
    }
    if (plane) *plane = words;
    return true;
}

inline uint64_t corr_words(const abnn_corr_config* c)
{
    uint64_t plane = 0;
    return corr_config_ok(c, &plane) ? ABNN_CORR_HEADER_WORDS + plane : 0;
}

// The handle's part of the checks: the ranges end inside N_NRN.
inline bool corr_ranges_ok(const abnn_corr_config& c, uint64_t n_nrn)
{
    return (uint64_t)c.a_first + c.a_count <= n_nrn && (uint64_t)c.b_first + c.b_count <= n_nrn;
}

// A config that passed the checks, as the rule reads it.
struct CorrRule {
    uint32_t a_first, a_count, b_first, b_count;  // count 0: every neuron
    uint64_t row_first, row_count;
    uint32_t L, mode, weight, n_nrn;
    float w_lo, w_hi;
};

inline CorrRule corr_rule(const abnn_corr_config& c, uint64_t n_nrn)
{
    return CorrRule{c.a_first, c.a_count, c.b_first, c.b_count, c.row_first, c.row_count, c.max_lag, c.mode,
                    c.flags & ABNN_CORR_WEIGHT, (uint32_t)n_nrn, c.w_lo, c.w_hi};
}

// The window [lo, hi) of table rows for K recorded rows (K already clamped to the pass capacity).
ABNN_CORR_HD inline void corr_window(const CorrRule& r, uint64_t K, uint64_t* lo, uint64_t* hi)
{
    const uint64_t first = r.row_first < K ? r.row_first : K;
    *lo = first;
    *hi = (r.row_count == 0 || r.row_count >= K - first) ? K : first + r.row_count;
}

// Row entry e clamped to a raster of `cap` entries: a corrupted table indexes nothing outside it.
ABNN_CORR_HD inline void corr_row(const abnn_spike_pass& e, uint64_t cap, uint64_t* off, uint32_t* count)
{
    const uint64_t o = e.offset < cap ? e.offset : cap;
    *off = o;
    *count = (uint64_t)e.count <= cap - o ? e.count : (uint32_t)(cap - o);
}

ABNN_CORR_HD inline bool corr_in_a(const CorrRule& r, uint32_t x)
{
    return x < r.n_nrn && (r.a_count == 0 || x - r.a_first < r.a_count);
}

ABNN_CORR_HD inline bool corr_in_b(const CorrRule& r, uint32_t x)
{
    return x < r.n_nrn && (r.b_count == 0 || x - r.b_first < r.b_count);
}

// Record {src, dst, w bits} is followed.
ABNN_CORR_HD inline bool corr_followed(const CorrRule& r, uint32_t src, uint32_t dst, uint32_t wbits)
{
    if (dst == kCorrTomb || !corr_in_a(r, src) || !corr_in_b(r, dst)) return false;
    if (!r.weight) return true;
    float w;
    __builtin_memcpy(&w, &wbits, 4);
    return w >= r.w_lo && w < r.w_hi;  // false for NaN
}

// The plane bin of the pair (row p, row q), lag q - p, or -1 when |q - p| > L.
ABNN_CORR_HD inline int32_t corr_bin(uint32_t L, uint64_t p, uint64_t q)
{
    const int64_t lag = (int64_t)q - (int64_t)p;
    return (lag + (int64_t)L >= 0 && lag <= (int64_t)L) ? (int32_t)(lag + L) : -1;
}

// The rule over a host pass table and raster (abnn_corr_host): the config has
// passed corr_config_ok and corr_ranges_ok, out holds corr_words(&c) u64.
inline void corr_host(const abnn_corr_config& c, uint64_t n_nrn, const abnn_spike_pass* passes, uint64_t K,
                      const uint32_t* raster, uint64_t cap, const abnn_synapse* rec, uint64_t n_rec, uint64_t* out)
{
    const CorrRule r = corr_rule(c, n_nrn);
    const uint64_t words = corr_words(&c), nb = 2ull * r.L + 1;
    for (uint64_t i = 0; i < words; ++i) out[i] = 0;
    uint64_t* plane = out + ABNN_CORR_HEADER_WORDS;
    uint64_t lo, hi;
    corr_window(r, K, &lo, &hi);
    out[0] = hi - lo;
    out[7] = K;
    std::vector<uint64_t> ca(hi - lo), cb(hi - lo);
    for (uint64_t p = lo; p < hi; ++p) {
        uint64_t off;
        uint32_t n;
        corr_row(passes[p], cap, &off, &n);
        out[1] += n;
        for (uint32_t i = 0; i < n; ++i) {
            ca[p - lo] += corr_in_a(r, raster[off + i]) ? 1 : 0;
            cb[p - lo] += corr_in_b(r, raster[off + i]) ? 1 : 0;
        }
        out[2] += ca[p - lo];
        out[3] += cb[p - lo];
    }
    if (r.mode == ABNN_CORR_POP) {
        for (uint64_t p = lo; p < hi; ++p)
            for (uint64_t q = (p - lo > r.L ? p - r.L : lo); q < hi && q <= p + r.L; ++q)
                plane[corr_bin(r.L, p, q)] += ca[p - lo] * cb[q - lo];
    } else if (r.mode == ABNN_CORR_PAIRS) {
        for (uint64_t p = lo; p < hi; ++p) {
            uint64_t po, qo;
            uint32_t pn, qn;
            corr_row(passes[p], cap, &po, &pn);
            if (ca[p - lo] == 0) continue;
            for (uint64_t q = (p - lo > r.L ? p - r.L : lo); q < hi && q <= p + r.L; ++q) {
                corr_row(passes[q], cap, &qo, &qn);
                const uint64_t bin = (uint64_t)corr_bin(r.L, p, q);
                for (uint32_t i = 0; i < pn; ++i) {
                    const uint32_t x = raster[po + i];
                    if (!corr_in_a(r, x)) continue;
                    for (uint32_t j = 0; j < qn; ++j) {
                        const uint32_t y = raster[qo + j];
                        if (corr_in_b(r, y)) plane[((uint64_t)(x - r.a_first) * r.b_count + (y - r.b_first)) * nb + bin] += 1;
                    }
                }
            }
        }
    } else {
        // the rows of every neuron's entries in the window, as lists (counting sort)
        std::vector<uint64_t> start(n_nrn + 1, 0);
        for (uint64_t p = lo; p < hi; ++p) {
            uint64_t off;
            uint32_t n;
            corr_row(passes[p], cap, &off, &n);
            for (uint32_t i = 0; i < n; ++i)
                if (raster[off + i] < n_nrn) start[raster[off + i] + 1] += 1;
        }
        for (uint64_t n = 0; n < n_nrn; ++n) start[n + 1] += start[n];
        std::vector<uint64_t> rows(start[n_nrn]), fill(start.begin(), start.end() - 1);
        for (uint64_t p = lo; p < hi; ++p) {
            uint64_t off;
            uint32_t n;
            corr_row(passes[p], cap, &off, &n);
            for (uint32_t i = 0; i < n; ++i)
                if (raster[off + i] < n_nrn) rows[fill[raster[off + i]]++] = p;
        }
        for (uint64_t k = 0; k < n_rec; ++k) {
            uint32_t wbits;
            __builtin_memcpy(&wbits, &rec[k].w, 4);
            if (!corr_followed(r, rec[k].src, rec[k].dst, wbits)) continue;
            out[5] += 1;
            uint64_t added = 0;
            for (uint64_t i = start[rec[k].src]; i < start[rec[k].src + 1]; ++i)
                for (uint64_t j = start[rec[k].dst]; j < start[rec[k].dst + 1]; ++j) {
                    const int32_t bin = corr_bin(r.L, rows[i], rows[j]);
                    if (bin >= 0) {
                        plane[bin] += 1;
                        added += 1;
                    }
                }
            out[6] += added ? 1 : 0;
        }
    }
    const uint64_t n_plane = words - ABNN_CORR_HEADER_WORDS;
    for (uint64_t i = 0; i < n_plane; ++i) out[4] += plane[i];
}

}  // namespace abnn

#if defined(__HIPCC__)
#include "engine.h"
#include "spikes.h"

namespace abnn {

constexpr int kCorrThreads = 512;        // k_corr_syn: 8 waves per workgroup
constexpr int kCorrUnroll = 2;           // 16-B lo + 8-B hi loads (8 records each) in flight per lane
constexpr int kCorrRowThreads = 256;     // k_corr_rows / k_corr_slabs / k_corr_pop / k_corr_pairs
constexpr uint32_t kCorrFoldWords = 8192;   // the map in LDS (32 KiB): whole up to 2^18 neurons, folded above (hops.h)
constexpr uint32_t kCorrQueue = 2048;       // k_corr_syn: staged double hits per workgroup iteration (16 KiB of LDS)
constexpr uint32_t kCorrLaneWalk = 64;      // ... a staged hit of at most this many pairs is walked by one lane
constexpr uint32_t kCorrChunk = 1024;       // k_corr_pairs: A-entries of a row held in LDS at a time
constexpr uint32_t kCorrBins = 2 * ABNN_CORR_MAX_LAG + 1;
static_assert(kCorrQueue % kCorrThreads == 0, "k_corr_syn's drain takes kCorrQueue / kCorrThreads staged hits per thread");

// A handle's correlogram scratch (capi.hip allocates it and frees it).
struct CorrScratch {
    uint32_t* map = nullptr;    // one bit per neuron: has a list (k_corr_slabs writes every word)
    uint32_t* cnt = nullptr;    // [N_NRN] entries of the neuron in the window = its list's length
    uint32_t* off = nullptr;    // [N_NRN] its list's first slot in `rows`
    uint32_t* cur = nullptr;    // [N_NRN] the fill cursor
    uint32_t* rows = nullptr;   // [raster_cap] the lists: row numbers relative to the window's first row
    uint2* tally = nullptr;     // [pass_cap] per row {entries in A, entries in B}
    uint32_t* cursor = nullptr; // [2] the slab cursor
    uint64_t raster_cap = 0;
    uint32_t pass_cap = 0;
};

inline uint64_t corr_map_words(uint64_t n_nrn) { return (n_nrn + 63) / 64 * 2; }

// Zeroes out_dev (corr_words u64) and fills it with the correlogram of the
// recorder `rec`'s raster (and, SYNAPSES, of records [0, n) of `a`), all in
// stream order on `s`; `cus` sizes the grids.  The config has passed
// corr_config_ok and corr_ranges_ok for n_nrn (< 2^32); the recorder has a raster.
hipError_t launch_corr(const SynArrays& a, uint64_t n, const abnn_corr_config& cfg, uint64_t n_nrn,
                       const SpikeRecorder& rec, const CorrScratch& scratch, uint64_t* out_dev, uint32_t cus,
                       hipStream_t s);

}  // namespace abnn
#endif
