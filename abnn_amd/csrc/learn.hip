// learn.hip -- the device-resident learning loop (abnn.h abnn_engine_*,
// DESIGN.md §9): BrainEngine::run_one_pass (brain-engine.cpp:108-190, restated
// in include/abnn/engine.hpp) around the traversal, without the host.
//
//   k_learn_boundary : one workgroup, launched between passes.  Its `post`
//       half is everything run_one_pass does after the traversal of pass p
//       (output read, rate EWMA, RateFilter, peak normalisation, the window's
//       loss -> reward, the trace); its `pre` half everything before the
//       traversal of pass p + 1 (input injection, teacher forcing).  Before a
//       call's first pass only pre runs, after its last only post.
//
// The arithmetic keeps engine.hpp's types and operation order (float EWMA,
// double filter coefficient, float FIR mean summed oldest first, double loss
// summed in index order), compiled with -ffp-contract=off, so a run is
// bit-identical to the host driver.  Both uniform streams are SplitMix64 with
// an additive state: draw k after state s is mix(s + (k + 1) * gamma), so
// every lane computes its own draw.
#include "learn.h"

#pragma clang fp contract(off)

namespace abnn {
namespace {

// SplitMix64 -> 24-bit uniform in [0, 1): draw k (0-based) after state s
// (capi.hip abnn_inject_inputs, engine.hpp BrainEngine::uni).
__device__ __forceinline__ float uni_at(uint64_t s, uint32_t k)
{
    uint64_t z = s + (uint64_t)(k + 1u) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (float)(z >> 40) * (1.0f / 16777216.0f);
}

}  // namespace

__global__ __launch_bounds__(kLearnThreads) void k_learn_boundary(LearnState st, LearnStep sp)
{
    __shared__ float red[kLearnThreads];
    const uint32_t tid = threadIdx.x;
    const uint32_t n_in = st.n_in, n_out = st.n_out;
    uint64_t* lf_out = st.last_fired + n_in;
    const uint64_t clk = *st.clock;  // stream order: after the last pass's tick (and renormalisation)
    LearnScalars sc = *st.sc;        // every lane's copy; lane 0 writes it back at the end

    if (sp.post_expected) {
        // read_outputs (brain.cpp:145-157) on u32 timestamps, as abnn_read_outputs
        const uint32_t now = (uint32_t)clk, start = now > 1 ? now - 1 : 0;
        const uint64_t step = sc.step;
        const uint32_t fs = st.fir_size;
        // RateFilter's ring after this frame is stored: it goes to slot step % fs,
        // the ring then holds n frames and its oldest is at `head`
        const uint32_t slot = st.use_fir ? (uint32_t)(step % fs) : 0;
        const uint32_t n = st.use_fir ? (uint32_t)(step + 1 < fs ? step + 1 : fs) : 0;
        const uint32_t head = st.use_fir && step + 1 > fs ? (uint32_t)((step + 1) % fs) : 0;
        const uint64_t tr = (step % st.trace_passes) * (uint64_t)n_out;
        const float a = st.rate_alpha;
        float m = sc.max_observed;
        for (uint32_t o = tid; o < n_out; o += kLearnThreads) {
            const uint32_t ts = (uint32_t)lf_out[o];
            const bool out = ts != 0 && ts >= start && ts < now;
            st.trace_out[tr + o] = out ? 1 : 0;
            st.spike_window[o] += out ? 1u : 0u;
            const float raw = (1 - a) * st.rate[o] + a * (out ? 1.f : 0.f);
            st.rate[o] = raw;
            float f = step == 0 ? raw : st.filt[o];  // the first frame initialises the state
            f += float(st.filt_a * (raw - f));
            st.filt[o] = f;
            float r = f;
            if (st.use_fir) {
                st.fir[(uint64_t)slot * n_out + o] = f;
                float mean = 0.0f;
                for (uint32_t k = 0; k < n; ++k) mean += st.fir[(uint64_t)((head + k) % n) * n_out + o];  // oldest first
                r = mean * (1.0f / float(n));
            }
            st.smooth[o] = r;
            m = m < r ? r : m;
        }
        // max_observed = max over every smooth rate (exact in any order), then its decay
        red[tid] = m;
        __syncthreads();
        for (uint32_t w = kLearnThreads / 2; w > 0; w >>= 1) {
            if (tid < w) red[tid] = red[tid] < red[tid + w] ? red[tid + w] : red[tid];
            __syncthreads();
        }
        const float mo = red[0] * st.peak_decay;
        for (uint32_t o = tid; o < n_out; o += kLearnThreads) {
            const float q = st.smooth[o] / mo;  // correctly rounded (HIP's default fp32 divide)
            const float r = 1.0f < q ? 1.0f : q;
            st.smooth[o] = r;
            st.trace_smooth[tr + o] = r;
        }
        sc.max_observed = mo;
        sc.step = step + 1;
        __syncthreads();  // lane 0 reads every smooth rate below; pre stamps what post read
        if (tid == 0 && ++sc.win_pos == st.win_size) {
            double loss = 0.0;
            for (uint32_t i = 0; i < n_out; ++i) {
                const double err = st.smooth[i] - sp.post_expected[i];
                loss += err * err;
            }
            loss /= n_out;
            sc.last_reward = float(sc.last_loss - loss);
            *st.reward = sc.last_reward;
            sc.last_loss = loss;
            sc.win_pos = 0;
            sc.windows += 1;
        }
    }

    if (sp.pre_in) {
        // inject_inputs (brain.cpp:73-83): lastFired[i] = clock iff uni < pTick * v[i]
        for (uint32_t i = tid; i < n_in; i += kLearnThreads)
            if (uni_at(sp.inject_state, i) < st.p_tick * sp.pre_in[i]) st.last_fired[i] = clk;
        // Poisson teacher forcing on every other pass (ENG:119-134); one draw per output
        const float teacher_rate = sc.teach ? 1.0f : 0.0f;
        for (uint32_t o = tid; o < n_out; o += kLearnThreads) {
            const float p = sp.pre_expected[o] * teacher_rate;
            const float u = uni_at(sp.teacher_state, o);
            if (u < p && (uint32_t)clk - (uint32_t)lf_out[o] > 1u) lf_out[o] = clk;
        }
        sc.teach = !sc.teach;
    }

    __syncthreads();  // every lane has its copy of the scalars
    if (tid == 0) *st.sc = sc;
}

hipError_t launch_learn_boundary(const LearnState& st, const LearnStep& step, hipStream_t s)
{
    hipLaunchKernelGGL(k_learn_boundary, dim3(1), dim3(kLearnThreads), 0, s, st, step);
    return hipGetLastError();
}

}  // namespace abnn
