// spikes.h -- the spike recorder (spikes.hip; abnn.h abnn_spikes_*, DESIGN.md
// §9): one small launch per pass that appends the pass's spike list to device
// buffers, as the C-ABI implementation (capi.hip) enqueues it from run_commit.
#pragma once

#include "engine.h"

namespace abnn {

constexpr int kSpikeThreads = 1024;  // one workgroup of 16 waves is the whole grid
constexpr int kSpikeWaves = kSpikeThreads / 64;

// The recorder's device words (u64), read by abnn_spikes_get_info: the seven
// words of abnn_spikes_info in order, then the sticky dropped flag.
constexpr uint32_t kSpikeWords = 8;
constexpr uint32_t kSpikeDroppedWord = 7;
static_assert(sizeof(abnn_spikes_info) == 7 * sizeof(uint64_t), "abnn_spikes_info is seven u64 words");
static_assert(sizeof(abnn_spike_pass) == 32 && sizeof(abnn_spikes_config) == 32, "abnn.h spike structs");

// A handle's recorder: the config it was started with and its device buffers.
struct SpikeRecorder {
    bool on = false;
    abnn_spikes_config cfg{};
    uint32_t first = 0;        // the counted neurons are [first, first + n_counts)
    uint64_t n_counts = 0;     // 0: counts off
    unsigned long long* words = nullptr;  // [kSpikeWords]
    abnn_spike_pass* passes = nullptr;    // [cfg.pass_capacity]
    uint32_t* raster = nullptr;           // [cfg.raster_capacity], null without a raster
    uint32_t* counts = nullptr;           // [n_counts], null with counts off
};

// Enqueues k_spike_record on `s` for the pass whose spike list is `list`
// (at most max_list entries, its length read on the device from *n_list).
// pass_index, now and epoch are the host mirrors' values before the pass's tick.
hipError_t launch_spike_record(const SpikeRecorder& r, const uint32_t* list, const uint32_t* n_list,
                               uint32_t max_list, uint64_t pass_index, uint64_t now, uint32_t epoch, hipStream_t s);

}  // namespace abnn
