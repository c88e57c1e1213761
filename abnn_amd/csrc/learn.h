// learn.h -- the device-resident learning loop's boundary kernel (learn.hip),
// as the C-ABI implementation (capi.hip, abnn_engine_*) launches it.
#pragma once

#include "engine.h"

namespace abnn {

// The driver's scalars (BrainEngine's members), one per engine, in device memory.
struct LearnScalars {
    unsigned long long step, windows, win_pos;
    double last_loss;
    float max_observed, last_reward;
    uint32_t teach;  // the reference's `even`: the NEXT pass teaches
    uint32_t pad;
};

// Kernel-facing view of an engine: the brain's words it reads and writes, its
// own arrays, the constants of its config.
struct LearnState {
    uint64_t* last_fired;  // the brain's [n_nrn]
    const uint64_t* clock;
    float* reward;
    LearnScalars* sc;
    float* rate;            // [n_out] EWMA of the output spikes
    float* filt;            // [n_out] the IIR filter's state
    float* fir;             // [fir_size][n_out] ring of filtered frames
    float* smooth;          // [n_out] the last pass's normalised rates
    uint32_t* spike_window; // [n_out]
    uint8_t* trace_out;     // [trace_passes][n_out]
    float* trace_smooth;    // [trace_passes][n_out]
    uint32_t n_in, n_out, use_fir, fir_size, win_size, trace_passes;
    float p_tick, rate_alpha, peak_decay;
    double filt_a;  // dt / (tau + dt)
};

// One boundary launch: post (the pass that just ran: its expected frame) and /
// or pre (the pass about to run: its frames, the RNG states before its draws).
struct LearnStep {
    const float* post_expected;  // null: no post half
    const float* pre_in;         // null: no pre half
    const float* pre_expected;
    uint64_t inject_state, teacher_state;
};

constexpr int kLearnThreads = 256;

hipError_t launch_learn_boundary(const LearnState& st, const LearnStep& step, hipStream_t s);

}  // namespace abnn
