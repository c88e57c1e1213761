// ubench_slice.hip -- does a fixed slice of the gate's record stream, read with
// ordinary loads while the rest stays non-temporal, get served from the
// Infinity Cache on the next launch?  The gate's stream at config-3 shape and
// nothing else: 256 workgroups x 1024 threads, one contiguous range of
// 512-event iterations per wave over 150,000,128 events, per iteration one
// 16-B load per lane from the 2 B/event array (syn.lo) and one 8-B load per
// lane from the 1 B/event array (syn.hi), two iterations in flight, the words
// folded into a value that is stored only under a condition that never holds.
//   nt       : both streams non-temporal (the product today)
//   plain    : both streams ordinary loads
//   slice k  : ordinary loads where (it & 15) < k, it the global iteration
//              index (the same lines every launch), non-temporal otherwise
//   slice k +traffic : and 450,000 random 8-B reads of a 40-MB table per
//              launch, in the waves' last two iterations (the gathers' share)
//   rot      : nt / plain, but every launch a wave starts a third of its own
//              range further back and wraps (how the cache treats a cyclic
//              stream; nothing in the product is built on it)
// Back-to-back launches: 64 to settle, 200 timed with one event pair.
//   hipcc --offload-arch=gfx950 -O3 -o tools/ubench_slice tools/ubench_slice.hip
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(x)                                                         \
    do {                                                              \
        hipError_t e = (x);                                           \
        if (e != hipSuccess) {                                        \
            printf("%s (line %d)\n", hipGetErrorString(e), __LINE__); \
            exit(1);                                                  \
        }                                                             \
    } while (0)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

enum { NT = 0, PLAIN = 1, SLICE = 2 };
constexpr uint32_t kReads = 450000, kTabBytes = 40000000;

__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct Args {
    const u32x4* lo;      // nit x 64 x 16 B
    const u32x2* hi;      // nit x 64 x 8 B
    const u32x4* dummy;   // 1 KiB of zeros: the block past a range's end
    const uint64_t* tab;  // kTabBytes, traffic variants only
    uint32_t* out;
    uint32_t nit;     // iterations of 512 events
    uint32_t k;       // SLICE: iterations with (it & 15) < k use ordinary loads
    uint32_t launch;  // launch index (rotation, the traffic's salt)
};

template <int POL, bool TRAFFIC, bool ROT>
__global__ __launch_bounds__(1024) void k_stream(Args a)
{
    const uint32_t lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t nwt = gridDim.x * 16, gw = blockIdx.x * 16 + wid;
    const uint32_t b0 = (uint32_t)((uint64_t)gw * a.nit / nwt), bend = (uint32_t)((uint64_t)(gw + 1) * a.nit / nwt);
    const uint32_t len = bend - b0;
    // rotated: this launch starts (launch % 3) thirds of the range back
    const uint32_t start = ROT && len ? (len - (uint32_t)((uint64_t)(a.launch % 3) * len / 3)) % len : 0;
    // The loads, their waits and the fold are inline asm.  Written as C++ the
    // compiler either merges the two flavours of a slice iteration into one
    // pair of ordinary loads, or, with the branch kept, no longer knows how
    // many loads are in flight and waits for all of them every trip
    // (s_waitcnt vmcnt(0) at the loop's head); with asm the loop is the same
    // for every variant: a slot is waited for with exactly the other slot's
    // two loads left in flight, folded, and refilled.
    u32x4 lo[2];
    u32x2 hi[2];
    auto issue = [&](int s, uint32_t j) __attribute__((always_inline)) {
        const bool live = j < len;
        uint32_t it = b0 + j;  // wave-uniform
        if (ROT) {
            it += start;
            if (it >= bend) it -= len;
        }
        const u32x4* pl = (live ? a.lo + (uint64_t)it * 64 : a.dummy) + lane;
        const u32x2* ph = (live ? a.hi + (uint64_t)it * 64 : reinterpret_cast<const u32x2*>(a.dummy)) + lane;
        const bool plain = POL == PLAIN || (POL == SLICE && (it & 15u) < a.k);
        // (early-clobber outputs: the second load's address must not share a
        // register with the first load's destination, which may land first)
        if (plain)
            asm volatile("global_load_dwordx4 %0, %2, off\n\tglobal_load_dwordx2 %1, %3, off"
                         : "=&v"(lo[s]), "=&v"(hi[s])
                         : "v"(pl), "v"(ph)
                         : "memory");
        else
            asm volatile("global_load_dwordx4 %0, %2, off nt\n\tglobal_load_dwordx2 %1, %3, off nt"
                         : "=&v"(lo[s]), "=&v"(hi[s])
                         : "v"(pl), "v"(ph)
                         : "memory");
    };
    uint32_t acc = 0;
    auto fold = [&](int s) __attribute__((always_inline)) {
        asm volatile("v_xor_b32 %0, %0, %1\n\tv_xor_b32 %0, %0, %2\n\tv_xor_b32 %0, %0, %3\n\t"
                     "v_xor_b32 %0, %0, %4\n\tv_xor_b32 %0, %0, %5\n\tv_xor_b32 %0, %0, %6"
                     : "+v"(acc)
                     : "v"(lo[s].x), "v"(lo[s].y), "v"(lo[s].z), "v"(lo[s].w), "v"(hi[s].x), "v"(hi[s].y));
    };
    uint64_t tv = 0;  // the traffic's word: waited for with the slot issued after it
    issue(0, 0);
    issue(1, 1);
    for (uint32_t j = 0; j < len; j += 2) {
        asm volatile("s_waitcnt vmcnt(2)" ::: "memory");  // in flight, oldest first: slot 0, slot 1
        fold(0);
        const bool tr = TRAFFIC && j + 4 >= len;  // the wave's last two trips (wave-uniform)
        if (tr) {
            // one random 8-B read per lane; 2 x 262,144 lanes a launch, 900,000 / 2^20
            // of them read the table (450,000 a launch), the others the dummy block
            const uint64_t u = ((uint64_t)a.launch << 32) | ((uint64_t)(j + 4 - len) << 24) | (gw * 64 + lane);
            const uint64_t h = mix64(u);
            const uint64_t* pt = (h & 0xFFFFFu) < 2u * kReads ? a.tab + __umul64hi(mix64(h), kTabBytes / 8)
                                                             : reinterpret_cast<const uint64_t*>(a.dummy);
            asm volatile("global_load_dwordx2 %0, %1, off" : "=&v"(tv) : "v"(pt) : "memory");
        }
        issue(0, j + 2);
        // in flight: slot 1, (the traffic's read,) slot 0
        if (tr)
            asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        else
            asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        fold(1);
        issue(1, j + 3);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the dummy blocks past the range, the traffic's last read
    asm volatile("v_xor_b32 %0, %0, %1" : "+v"(acc) : "v"((uint32_t)tv));
    if (acc == 0x12345678u) a.out[blockIdx.x] = acc;
}

typedef void (*Kern)(Args);
struct V {
    const char* name;
    Kern kern;
    uint32_t k;
    std::vector<float> us;
};

static float run(Kern kern, Args a)
{
    static hipEvent_t e0, e1;
    static uint32_t launch = 0;
    if (!e0) {
        CK(hipEventCreate(&e0));
        CK(hipEventCreate(&e1));
    }
    for (int i = 0; i < 64; ++i) {
        a.launch = launch++;
        hipLaunchKernelGGL(kern, dim3(256), dim3(1024), 0, 0, a);
    }
    CK(hipEventRecord(e0));
    for (int i = 0; i < 200; ++i) {
        a.launch = launch++;
        hipLaunchKernelGGL(kern, dim3(256), dim3(1024), 0, 0, a);
    }
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    CK(hipGetLastError());
    float ms;
    CK(hipEventElapsedTime(&ms, e0, e1));
    return ms * 1000.0f / 200.0f;
}

int main(int argc, char** argv)
{
    const uint64_t events = 150000128ull;  // config 3; a multiple of 512
    const uint32_t nit = (uint32_t)(events / 512);
    char *lo, *hi, *dummy, *tab;
    uint32_t* out;
    CK(hipMalloc(&lo, (uint64_t)nit * 1024));
    CK(hipMalloc(&hi, (uint64_t)nit * 512));
    CK(hipMalloc(&dummy, 1024));
    CK(hipMalloc(&tab, kTabBytes));
    CK(hipMalloc(&out, 256 * 4));
    CK(hipMemset(lo, 1, (uint64_t)nit * 1024));
    CK(hipMemset(hi, 1, (uint64_t)nit * 512));
    CK(hipMemset(dummy, 0, 1024));
    CK(hipMemset(tab, 1, kTabBytes));
    Args a{(const u32x4*)lo, (const u32x2*)hi, (const u32x4*)dummy, (const uint64_t*)tab, out, nit, 0, 0};

    std::vector<V> vs = {
        {"nt", k_stream<NT, false, false>, 0, {}},
        {"plain", k_stream<PLAIN, false, false>, 16, {}},
        {"slice k=0", k_stream<SLICE, false, false>, 0, {}},
        {"slice k=2", k_stream<SLICE, false, false>, 2, {}},
        {"slice k=4", k_stream<SLICE, false, false>, 4, {}},
        {"slice k=5", k_stream<SLICE, false, false>, 5, {}},
        {"slice k=6", k_stream<SLICE, false, false>, 6, {}},
        {"slice k=8", k_stream<SLICE, false, false>, 8, {}},
        {"nt +traffic", k_stream<NT, true, false>, 0, {}},
        {"slice k=2 +traffic", k_stream<SLICE, true, false>, 2, {}},
        {"slice k=4 +traffic", k_stream<SLICE, true, false>, 4, {}},
        {"slice k=5 +traffic", k_stream<SLICE, true, false>, 5, {}},
        {"slice k=6 +traffic", k_stream<SLICE, true, false>, 6, {}},
        {"slice k=8 +traffic", k_stream<SLICE, true, false>, 8, {}},
        {"rot nt", k_stream<NT, false, true>, 0, {}},
        {"rot plain", k_stream<PLAIN, false, true>, 16, {}},
    };
    const int rounds = argc > 1 ? std::max(1, atoi(argv[1])) : 5;  // interleaved: every variant once per round
    for (int r = 0; r < rounds; ++r)
        for (V& v : vs) {
            a.k = v.k;
            v.us.push_back(run(v.kern, a));
        }
    const double bytes = (double)nit * 1536.0;
    printf("ubench_slice: %llu events, %u iterations, %.1f MB of stream; 256 x 1024 threads; per variant %d repeats of "
           "64 settling + 200 timed launches, interleaved\n",
           (unsigned long long)events, nit, bytes / 1e6, rounds);
    printf("%-20s %9s %9s %9s %9s   repeats (us)\n", "variant", "median us", "min", "max", "GB/s");
    std::vector<double> med(vs.size());
    for (size_t i = 0; i < vs.size(); ++i) {
        std::vector<float> s = vs[i].us;
        std::sort(s.begin(), s.end());
        med[i] = s[s.size() / 2];
        printf("%-20s %9.2f %9.2f %9.2f %9.0f  ", vs[i].name, med[i], s.front(), s.back(), bytes / (med[i] * 1e3));
        for (float u : vs[i].us) printf(" %.2f", u);
        printf("\n");
    }
    const auto mm = std::minmax_element(vs[0].us.begin(), vs[0].us.end());
    const double spread = *mm.second - *mm.first;
    printf("nt spread (max - min of its repeats) %.2f us\n", spread);
    // best slice of vs[first..last] against vs[base]
    auto decide = [&](size_t base, size_t first, size_t last) {
        size_t best = first;
        for (size_t i = first; i <= last; ++i)
            if (med[i] < med[best]) best = i;
        const double gain = med[base] - med[best];
        printf("best '%s' is %.2f us %s than '%s': %s\n", vs[best].name, gain < 0 ? -gain : gain,
               gain < 0 ? "slower" : "faster", vs[base].name,
               gain > 3.0 * spread ? "GO (more than 3 x spread)" : "STOP (not more than 3 x spread)");
    };
    decide(0, 3, 7);
    decide(8, 9, 13);
    return 0;
}
