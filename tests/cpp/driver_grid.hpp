// driver_grid.hpp -- TEST CODE (CPU only): one harness over two implementations
// of the learning driver's host classes.  tests/cpp/engine_host_test.cpp runs
// it on include/abnn/engine.hpp's RateFilter / FunctionalDataset,
// oracle/ref_recipe/ref_driver.cpp on the reference's own classes; the two
// JSON documents must be equal (tests/test_engine.py).  Floats are printed as
// their u32 bits; long vectors as a chained 64-bit FNV-1a hash over those bits,
// so equal documents mean equal bits in every float of every frame.
//
// Grid: RateFilter with tau in {0.02, 0.05}, FIR off and on with windows 1, 5
// and 20, vectors of 1, 8 and 257 values over 45 frames (the 20-frame ring
// wraps more than twice); FunctionalDataset at 8/8 and 256/256 over 2300
// frames of dt = 0.0009 at 0.5 Hz (the phase passes 1.0 at frame 2222).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace driver_grid {

struct Fnv {
    uint64_t h = 0xCBF29CE484222325ull;
    void add(const std::vector<float>& v)
    {
        for (float x : v) {
            unsigned char b[4];
            std::memcpy(b, &x, 4);
            for (int k = 0; k < 4; ++k) h = (h ^ b[k]) * 0x100000001B3ull;
        }
    }
};

inline uint32_t bits(float x)
{
    uint32_t u;
    std::memcpy(&u, &x, 4);
    return u;
}

// the values at the vector's two ends (all of a short vector)
inline void print_ends(const std::vector<float>& v)
{
    std::printf("[");
    bool first = true;
    for (size_t i = 0; i < v.size(); ++i)
        if (v.size() <= 8 || i < 4 || i + 4 >= v.size()) {
            std::printf("%s%u", first ? "" : ", ", bits(v[i]));
            first = false;
        }
    std::printf("]");
}

inline float raw_value(int f, size_t i)
{
    return float((f * 7 + int(i) * 3) % 5) * 0.25f + float((f * f + int(i)) % 7) * 0.03125f;
}

template <class Filter> void print_filters()
{
    const double taus[2] = {0.02, 0.05};
    const int modes[4] = {0, 1, 5, 20};  // 0: FIR off, else the window
    const size_t lens[3] = {1, 8, 257};
    bool first = true;
    for (double tau : taus)
        for (int mode : modes)
            for (size_t len : lens) {
                Filter flt(tau, mode != 0, size_t(mode ? mode : 20));
                Fnv h;
                std::printf("%s{\"tau\": %.17g, \"fir\": %d, \"len\": %zu, \"hash\": [", first ? "" : ", ", tau, mode, len);
                first = false;
                std::vector<float> out;
                for (int f = 0; f < 45; ++f) {
                    std::vector<float> raw(len);
                    for (size_t i = 0; i < len; ++i) raw[i] = raw_value(f, i);
                    out = flt.process(raw, f % 3 == 2 ? 0.0011 : 0.0009);
                    h.add(out);
                    // around the frames at which the windows of 5 and 20 fill and wrap
                    if (f == 0 || f == 4 || f == 5 || f == 19 || f == 20 || f == 40 || f == 44) std::printf("%s%llu", f ? ", " : "", (unsigned long long)h.h);
                }
                std::printf("], \"last\": ");
                print_ends(out);
                std::printf("}");
            }
}

template <class Dataset, class Fn> void print_datasets(Fn f_in, Fn f_ex)
{
    const uint32_t sizes[2] = {8, 256};
    for (int s = 0; s < 2; ++s) {
        const uint32_t n = sizes[s];
        Dataset ds(n, n, 0.0009, 0.5, f_in, f_ex);
        Fnv hi, he;
        std::printf("%s{\"n\": %u, \"frames\": [", s ? ", " : "", n);
        bool first = true;
        for (int f = 0; f < 2300; ++f) {
            const std::vector<float> in = ds.nextInput(), ex = ds.nextExpected();
            hi.add(in);
            he.add(ex);
            const bool shown = f < 2 || (f >= 2220 && f <= 2225) || f == 2299;
            if (shown || f % 100 == 0) {
                const double t = ds.time();
                uint64_t tb;
                std::memcpy(&tb, &t, 8);
                std::printf("%s{\"f\": %d, \"in_hash\": %llu, \"ex_hash\": %llu, \"time_bits\": %llu", first ? "" : ", ", f,
                            (unsigned long long)hi.h, (unsigned long long)he.h, (unsigned long long)tb);
                first = false;
                if (shown) {
                    std::printf(", \"in\": ");
                    print_ends(in);
                    std::printf(", \"ex\": ");
                    print_ends(ex);
                }
                std::printf("}");
            }
        }
        std::printf("], \"time\": %.17g}", ds.time());
    }
}

template <class Filter, class Dataset, class Fn> void print_all(Fn f_in, Fn f_ex)
{
    std::printf("{\"filter\": [");
    print_filters<Filter>();
    std::printf("], \"dataset\": [");
    print_datasets<Dataset>(f_in, f_ex);
    std::printf("]}\n");
}

}  // namespace driver_grid
