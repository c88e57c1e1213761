// spikes.hip -- the spike recorder (abnn.h abnn_spikes_*).
//
//   k_spike_record<kRange> : one workgroup, one launch per pass, in stream
//       order after the pass's kernels.  It reads the pass's spike list L (the
//       fired_ring slot, its length from n_fired_ring: the host never knows it)
//       and applies the per-pass rule of abnn.h: the *_seen words, the
//       per-neuron counts, then either the pass entry and S appended to the
//       raster, or the pass dropped whole and the sticky flag set.
//
// Two sweeps over L.  The first counts |S| (and adds the per-neuron counts:
// global u32 atomics without a return value), so that the room is decided
// before any raster entry is written.  The second writes S: without a range a
// plain copy (kRange = false, no test per spike); with one, chunk by chunk of
// kSpikeThreads entries, a wave64 ballot per wave, the waves' popcounts through
// LDS, and each selected lane's slot = running base + the lower waves' counts +
// its rank among the wave's selected lanes, so S keeps L's order.  The list was
// just written by the pass, so the second sweep reads it from L2.
//
// The cursors live in device memory (r.words) and only this kernel and the
// host's clear (after a synchronise) write them: launches on one stream are
// serial, and a single workgroup waits on nothing.  Every word is an integer.
#include "spikes.h"

namespace abnn {
namespace {

struct SpikeArgs {
    const uint32_t* list;
    const uint32_t* n_list;
    uint32_t max_list;
    unsigned long long* words;
    abnn_spike_pass* passes;
    uint32_t* raster;  // null: no raster
    uint32_t* counts;  // null: counts off
    uint64_t raster_capacity;
    uint64_t n_counts;
    uint32_t pass_capacity;
    uint32_t first, span;  // kRange: dst is selected iff dst - first < span; counts index dst - first
    uint64_t pass_index, now;
    uint32_t epoch;
};

template <bool kRange>
__global__ __launch_bounds__(kSpikeThreads) void k_spike_record(SpikeArgs a)
{
    __shared__ uint32_t s_red[kSpikeWaves], s_wave[kSpikeWaves];
    constexpr uint32_t T = kSpikeThreads;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    uint32_t n = *a.n_list;
    n = n < a.max_list ? n : a.max_list;
    // the cursors, read by every thread before thread 0 rewrites them (below, after a barrier)
    const uint64_t rec_p = a.words[3], rec_s = a.words[4];
    const bool dropped = a.words[kSpikeDroppedWord] != 0;

    // sweep 1: |S|, and the counts
    uint32_t sel = n;
    if (kRange) {
        uint32_t mine = 0;
        for (uint32_t i = tid; i < n; i += T) {
            const uint32_t k = a.list[i] - a.first;
            if (k < a.span) {
                ++mine;
                if (a.counts) __hip_atomic_fetch_add(a.counts + k, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        for (int m = 32; m > 0; m >>= 1) mine += __shfl_xor(mine, m);
        if (lane == 0) s_red[wid] = mine;
        __syncthreads();
        sel = 0;
        for (uint32_t w = 0; w < (uint32_t)kSpikeWaves; ++w) sel += s_red[w];
    } else {
        if (a.counts)
            for (uint32_t i = tid; i < n; i += T) {
                const uint32_t d = a.list[i];  // a spike's dst is a neuron id: the test only guards the buffer
                if (d < a.n_counts) __hip_atomic_fetch_add(a.counts + d, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        __syncthreads();
    }

    const bool rec = !dropped && rec_p < a.pass_capacity &&
                     (a.raster_capacity == 0 || rec_s + sel <= a.raster_capacity);

    // sweep 2: S appended at rec_s, in L's order
    if (rec && a.raster) {
        if (kRange) {
            uint64_t base = rec_s;
            for (uint32_t c0 = 0; c0 < n; c0 += T) {  // workgroup-uniform
                const uint32_t i = c0 + tid;
                const uint32_t d = i < n ? a.list[i] : 0u;
                const bool in = i < n && d - a.first < a.span;
                const unsigned long long ballot = __ballot(in);
                if (lane == 0) s_wave[wid] = (uint32_t)__popcll(ballot);
                __syncthreads();
                uint32_t below = 0, total = 0;
                for (uint32_t w = 0; w < (uint32_t)kSpikeWaves; ++w) {
                    const uint32_t v = s_wave[w];
                    below += w < wid ? v : 0u;
                    total += v;
                }
                if (in) a.raster[base + below + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull))] = d;
                base += total;
                __syncthreads();  // s_wave is rewritten by the next chunk
            }
        } else {
            for (uint32_t i = tid; i < n; i += T) a.raster[rec_s + i] = a.list[i];
        }
    }

    if (tid == 0) {
        a.words[0] += 1;
        a.words[1] += n;
        a.words[2] += sel;
        if (rec) {
            abnn_spike_pass e;
            e.pass_index = a.pass_index;
            e.now = a.now;
            e.offset = rec_s;
            e.count = sel;
            e.epoch = a.epoch;
            a.passes[rec_p] = e;
            a.words[3] = rec_p + 1;
            a.words[4] = rec_s + sel;
        } else {
            a.words[5] += 1;
            a.words[6] += sel;
            a.words[kSpikeDroppedWord] = 1;
        }
    }
}

}  // namespace

hipError_t launch_spike_record(const SpikeRecorder& r, const uint32_t* list, const uint32_t* n_list,
                               uint32_t max_list, uint64_t pass_index, uint64_t now, uint32_t epoch, hipStream_t s)
{
    SpikeArgs a{};
    a.list = list;
    a.n_list = n_list;
    a.max_list = max_list;
    a.words = r.words;
    a.passes = r.passes;
    a.raster = r.raster;
    a.counts = r.counts;
    a.raster_capacity = r.cfg.raster_capacity;
    a.n_counts = r.n_counts;
    a.pass_capacity = r.cfg.pass_capacity;
    a.first = r.cfg.count ? r.cfg.first : 0u;
    a.span = r.cfg.count;
    a.pass_index = pass_index;
    a.now = now;
    a.epoch = epoch;
    if (r.cfg.count)
        hipLaunchKernelGGL(k_spike_record<true>, dim3(1), dim3(kSpikeThreads), 0, s, a);
    else
        hipLaunchKernelGGL(k_spike_record<false>, dim3(1), dim3(kSpikeThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace abnn
