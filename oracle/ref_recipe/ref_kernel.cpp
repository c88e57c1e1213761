// ref_kernel.cpp -- the reference's kernel file, compiled in place as host C++
// behind the stand-in metal_stdlib of this directory, and run one dispatch at
// a time under schedule C1.  TEST INFRASTRUCTURE ONLY:
// built by abnn_amd/build.py: build_reference() into oracle/_ref/ (never
// committed), loaded with ctypes by tests/ref_kernel_helpers.py.
//
// The reference file is included by name through -I <checkout>/abnn/src; no
// line of it is copied, patched or generated here.
#include <cstdint>
#include <cstring>
#include <vector>

#include <metal_stdlib>

#include "core/kernels/brain.metal"

#undef kernel
#undef device
#undef constant
#undef threadgroup

namespace {

template <class T> std::vector<metal::c1_cell<T>> cells(const T* v, size_t n)
{
    std::vector<metal::c1_cell<T>> c(n);
    for (size_t i = 0; i < n; ++i) c[i] = {v[i], v[i], false};
    return c;
}

inline uint32_t grid_of(uint32_t n) { return (n + 255u) / 256u * 256u; }  // brain.cpp:116-118, 137-139

}  // namespace

extern "C" {

// One dispatch of monte_carlo_traversal as Brain::encode_traversal issues it
// (brain.cpp:93-118): roundup(events, 256) threads in groups of 256, called
// thread by thread in tid order; pending stores land when the dispatch ends.
// syn16: n_syn 16-B SynapsePacked records.  scal = {clock, budget, reward
// bits, rBar bits}, all updated in place (the budget is what the host left
// there: the caller resets it, brain.cpp:90).
void ref_pass(void* syn16, uint32_t* lastF, uint32_t n_nrn, uint32_t* scal, uint32_t n_syn, uint32_t events,
              float aLTP, float aLTD, float wMin, float wMax)
{
    std::vector<atomic_uint> lf = cells<uint>(lastF, n_nrn), lv(n_nrn, atomic_uint{0u, 0u, false});
    atomic_uint clock = {scal[0], scal[0], false};
    atomic_uint budget = {scal[1], scal[1], true};  // sequentially consistent in tid order
    float reward, rbar;
    std::memcpy(&reward, &scal[2], 4);
    std::memcpy(&rbar, &scal[3], 4);
    atomic_float rbar_cell = {rbar, rbar, false};
    const uint tau_vis = 50000u, tau_pre = 50000u;  // brain.cpp:102
    const uint3 tg_size = {256u, 1u, 1u};
    const uint32_t grid = grid_of(events);
    for (uint32_t tid = 0; tid < grid; ++tid) {
        const uint3 t_pos = {tid % 256u, 0u, 0u}, g_pos = {tid, 0u, 0u};
        monte_carlo_traversal(static_cast<SynapsePacked*>(syn16), lf.data(), lv.data(), &clock, n_syn, tau_vis,
                              tau_pre, aLTP, aLTD, wMin, wMax, &budget, &reward, &rbar_cell, t_pos, g_pos, tg_size);
    }
    for (uint32_t i = 0; i < n_nrn; ++i) lastF[i] = lf[i].pending;
    scal[0] = clock.pending;
    scal[1] = budget.pending;
    std::memcpy(&scal[3], &rbar_cell.pending, 4);
}

// One dispatch of renormalise_clock_and_times (brain.cpp:130-140).
void ref_renormalise(uint32_t* lastF, uint32_t* clock, uint32_t n_nrn)
{
    std::vector<atomic_uint> lf = cells<uint>(lastF, n_nrn), lv(n_nrn, atomic_uint{0u, 0u, false});
    atomic_uint clk = {*clock, *clock, false};
    const uint32_t grid = grid_of(n_nrn);
    for (uint32_t tid = 0; tid < grid; ++tid) renormalise_clock_and_times(lf.data(), lv.data(), &clk, n_nrn, tid);
    for (uint32_t i = 0; i < n_nrn; ++i) lastF[i] = lf[i].pending;
    *clock = clk.pending;
}

}  // extern "C"
