// runs.h -- run aggregation along a wave's consecutive records,
// lifted from the degree census's scatter() (degree.hip) for the kernels that
// add one 64-bit value per record to a keyed accumulator.  Device inlines only.
//
// A wave's 128 records of one scan.h load are consecutive (lane l holds records
// 2l and 2l + 1), so keys that repeat in consecutive records (the generated
// graph's dense block: 256 records per src; a sorted upload; every record on
// one neuron) form runs along the lanes.  scatter_runs() turns every run into
// ONE emit of the run's sum (modulo 2^64) by the run's first lane: the two
// records of a lane merge first; a lane whose records differ hands its first
// record to the lane before it when that lane ends on the same key; then each
// lane holds one item, run heads are found with one ballot, and a wave prefix
// sum gives each head its run's total (last lane's prefix minus its own).  A
// wave with no item skips all of it, and a wave whose items are all different
// skips the scan.  k_degree keeps its own copy (two sums packed in one word):
// its code is pinned by its measurements.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace abnn {

constexpr uint32_t kRunNone = 0xFFFFFFFFu;    // no item: a record that adds nothing, no record
constexpr uint32_t kRunNoPush = 0xFFFFFFFEu;  // "this lane hands nothing back"

struct RunItem {
    uint32_t key;  // the accumulator's index, or kRunNone
    uint64_t v;
};

// Cross-lane moves on the VALU (DPP), every lane of the wave active: a lane
// with no source lane gets 0.  Controls: row_shr:n = 0x110 + n (lane l of a
// 16-lane row reads lane l - n), wave_shl:1 / wave_shr:1 (lane l reads lane
// l + 1 / l - 1 of the wave), row_bcast:15 / :31 (lane 15 / 31 to the whole
// next row / the upper half; the row mask names the rows that receive).
constexpr int kRunDppWaveShl1 = 0x130, kRunDppWaveShr1 = 0x138, kRunDppBcast15 = 0x142, kRunDppBcast31 = 0x143;

template <int kCtrl, int kRows = 0xF>
__device__ __forceinline__ uint32_t run_dpp(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kCtrl, kRows, 0xF, false);
}

template <int kCtrl, int kRows = 0xF>
__device__ __forceinline__ uint64_t run_dpp(uint64_t v)
{
    return (uint64_t)run_dpp<kCtrl, kRows>((uint32_t)v) | (uint64_t)run_dpp<kCtrl, kRows>((uint32_t)(v >> 32)) << 32;
}

// inclusive prefix sum over the wave's 64 lanes, modulo 2^64
__device__ __forceinline__ uint64_t run_wave_prefix(uint64_t v)
{
    // a lane without a source lane (the row's first n, the rows outside the mask) adds the 0 it got
    v += run_dpp<0x111>(v);
    v += run_dpp<0x112>(v);
    v += run_dpp<0x114>(v);
    v += run_dpp<0x118>(v);
    v += run_dpp<kRunDppBcast15, 0xA>(v);
    v += run_dpp<kRunDppBcast31, 0xC>(v);
    return v;
}

// The wave's items of one load: lane l holds those of records 2l (r0) and
// 2l + 1 (r1).  Every lane of the wave calls it; emit(key, sum) is called once
// per run, by one lane, with key != kRunNone.
template <typename Emit>
__device__ __forceinline__ void scatter_runs(uint32_t lane, RunItem r0, RunItem r1, Emit emit)
{
    if (!__any(r0.key != kRunNone || r1.key != kRunNone)) return;
    const bool uni = r0.key == r1.key;
    uint64_t tv = uni ? r0.v + r1.v : r1.v;  // the lane's item has key r1.key
    // lane 0's prev_tail and lane 63's next_* are not used
    const uint32_t prev_tail = run_dpp<kRunDppWaveShr1>(r1.key);
    const uint32_t next_head = run_dpp<kRunDppWaveShl1>(uni ? kRunNoPush : r0.key);
    const uint64_t next_v = run_dpp<kRunDppWaveShl1>(r0.v);
    if (lane < 63 && next_head == r1.key && r1.key != kRunNone) tv += next_v;
    const bool handed = !uni && lane > 0 && prev_tail == r0.key;
    if (!uni && !handed && r0.key != kRunNone) emit(r0.key, r0.v);
    const bool head = lane == 0 || !uni || prev_tail != r1.key;
    const uint64_t heads = __ballot(head);
    if (heads == ~0ull) {
        if (r1.key != kRunNone) emit(r1.key, tv);
        return;
    }
    const uint64_t p = run_wave_prefix(tv);
    if (heads == 1ull) {  // the wave is one run: its total is the last lane's prefix
        const uint64_t total = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)p, 63) |
                               (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(p >> 32), 63) << 32;
        if (lane == 0 && r1.key != kRunNone) emit(r1.key, total);
        return;
    }
    const uint64_t above = lane == 63 ? 0ull : heads & (~0ull << (lane + 1));
    const uint32_t last = above ? (uint32_t)__ffsll((unsigned long long)above) - 2u : 63u;  // the run's last lane
    const uint64_t pe = __shfl((unsigned long long)p, (int)last);
    if (head && r1.key != kRunNone) emit(r1.key, pe - p + tv);
}

}  // namespace abnn
