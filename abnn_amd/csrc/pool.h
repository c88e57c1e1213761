// pool.h -- who owns device memory in the C-ABI implementation (capi.hip,
// DESIGN.md §9 "Device memory").  Every hipMalloc of capi.hip is made here, by
// one of two owners: a DevicePool, one per handle (abnn_brain, abnn_snapshot,
// abnn_engine, abnn_comm), which remembers what it allocated and frees it with
// the handle; or a DeviceTemp, freed at the end of its scope.  The structs that
// kernels receive by value (DeviceState, SynArrays, the modules' scratch) stay
// plain structs of raw pointers: the pool sits beside them and fills them in.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/abnn/abnn.h"

namespace abnn {

void set_err(const std::string& m);  // capi.hip: the calling thread's abnn_last_error

// Allocations made here and not freed yet, process-wide (abnn_debug_live_allocations).
inline std::atomic<uint64_t> g_live_allocations{0};

// The one hipMalloc: `bytes` at *p, zeroed or as they come.  ABNN_ERR_OOM when
// the memory is not there (*p is null then).
inline abnn_status device_malloc(void** p, uint64_t bytes, bool zeroed)
{
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) {
        *p = nullptr;
        (void)hipGetLastError();
        set_err(std::string("hipMalloc(") + std::to_string(bytes) + " B): " + hipGetErrorString(e));
        return ABNN_ERR_OOM;
    }
    g_live_allocations.fetch_add(1, std::memory_order_relaxed);
    if (zeroed && (e = hipMemset(*p, 0, bytes)) != hipSuccess) {
        set_err(std::string("hipMemset: ") + hipGetErrorString(e));
        return ABNN_ERR_HIP;
    }
    return ABNN_OK;
}

// ... and the one hipFree.
inline void device_free(void* p)
{
    if (p && hipFree(p) == hipSuccess) g_live_allocations.fetch_sub(1, std::memory_order_relaxed);
}

// A buffer to allocate: `count` entries at *p (an empty buffer is one entry
// long, so its pointer is never null), zeroed, or raw: no memset, for buffers
// whose kernels write every word before they read it.
struct Slot {
    void** p;
    uint64_t bytes;
    bool zeroed;
};
template <typename T>
Slot zeroed(T** p, uint64_t count) { return {reinterpret_cast<void**>(p), std::max<uint64_t>(count, 1) * sizeof(T), true}; }
template <typename T>
Slot raw(T** p, uint64_t count) { return {reinterpret_cast<void**>(p), std::max<uint64_t>(count, 1) * sizeof(T), false}; }

class DevicePool {
public:
    DevicePool() = default;
    DevicePool(const DevicePool&) = delete;
    DevicePool& operator=(const DevicePool&) = delete;
    ~DevicePool() { release_all(); }

    // A failed memset leaves the buffer with the pool, to be released with the rest.
    abnn_status alloc(const Slot& s)
    {
        const abnn_status st = device_malloc(s.p, s.bytes, s.zeroed);
        if (*s.p) owned_.push_back(*s.p);
        return st;
    }

    // All of the slots (null on entry) or none: the first failure releases
    // the ones that were filled, so every one of them is null again.
    abnn_status alloc_all(const std::vector<Slot>& slots)
    {
        for (const Slot& s : slots) {
            const abnn_status st = alloc(s);
            if (st == ABNN_OK) continue;
            for (const Slot& u : slots) release(u.p);
            return st;
        }
        return ABNN_OK;
    }

    // A buffer that grows to the largest count asked: *p holds *cap entries.
    template <typename T, typename Cap>
    abnn_status grow(T** p, Cap* cap, uint64_t count, bool zero = true)
    {
        if (count <= *cap) return ABNN_OK;
        release(p);
        *cap = 0;
        const abnn_status st = alloc(zero ? zeroed(p, count) : raw(p, count));
        if (st == ABNN_OK) *cap = static_cast<Cap>(count);
        return st;
    }

    // Frees each *p now (null: nothing), forgets it and nulls the caller's pointer.
    template <typename... T>
    void release(T**... p) { (release_one(reinterpret_cast<void**>(p)), ...); }

    // Frees everything the pool still owns: a handle's destroy, on the handle's device.
    void release_all()
    {
        for (void* v : owned_) device_free(v);
        owned_.clear();
    }

private:
    void release_one(void** p)
    {
        const auto it = std::find(owned_.begin(), owned_.end(), *p);
        if (it != owned_.end()) {
            device_free(*it);
            *it = owned_.back();
            owned_.pop_back();
        }
        *p = nullptr;
    }

    std::vector<void*> owned_;
};

// A device buffer that lives for one call: freed when it leaves scope.
template <typename T>
struct DeviceTemp {
    T* dev = nullptr;
    DeviceTemp() = default;
    DeviceTemp(const DeviceTemp&) = delete;
    DeviceTemp& operator=(const DeviceTemp&) = delete;
    ~DeviceTemp() { device_free(dev); }
    abnn_status alloc(uint64_t count, bool zero = true)
    {
        const Slot s = zero ? zeroed(&dev, count) : raw(&dev, count);
        return device_malloc(s.p, s.bytes, s.zeroed);
    }
};

}  // namespace abnn
