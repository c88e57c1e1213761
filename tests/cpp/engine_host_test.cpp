// engine_host_test.cpp -- TEST PROGRAM (CPU only): RateFilter and
// FunctionalDataset of include/abnn/engine.hpp on fixed inputs; the output is
// compared with an independent numpy restatement in tests/test_engine.py.
// With the argument "grid": the grid of driver_grid.hpp instead, compared with
// the same grid run on the reference's own classes (oracle/ref_recipe/
// ref_driver.cpp, recorded in tests/golden/ref_driver.json).
#include <abnn/engine.hpp>

#include <cstdio>
#include <cstring>

#include "driver_grid.hpp"

int main(int argc, char** argv)
{
    if (argc > 1 && std::strcmp(argv[1], "grid") == 0) {
        driver_grid::print_all<abnn::RateFilter, abnn::FunctionalDataset>(&abnn::FunctionalDataset::cos_squared,
                                                                          &abnn::FunctionalDataset::half_sine);
        return 0;
    }
    abnn::FunctionalDataset ds(8, 8, 0.0009, 0.5, abnn::FunctionalDataset::cos_squared,
                               abnn::FunctionalDataset::half_sine);
    abnn::RateFilter iir(0.02, false), fir(0.02, true, 5);
    std::printf("{\"frames\": [");
    for (int f = 0; f < 12; ++f) {
        const std::vector<float> in = ds.nextInput(), ex = ds.nextExpected();
        std::vector<float> raw(8);
        for (int i = 0; i < 8; ++i) raw[i] = ((f * 7 + i * 3) % 5) * 0.25f;
        const std::vector<float> a = iir.process(raw, 0.0009), b = fir.process(raw, 0.0009);
        std::printf("%s{\"in\": [", f ? ", " : "");
        for (int i = 0; i < 8; ++i) std::printf("%s%.9g", i ? ", " : "", in[i]);
        std::printf("], \"ex\": [");
        for (int i = 0; i < 8; ++i) std::printf("%s%.9g", i ? ", " : "", ex[i]);
        std::printf("], \"iir\": [");
        for (int i = 0; i < 8; ++i) std::printf("%s%.9g", i ? ", " : "", a[i]);
        std::printf("], \"fir\": [");
        for (int i = 0; i < 8; ++i) std::printf("%s%.9g", i ? ", " : "", b[i]);
        std::printf("]}");
    }
    std::printf("], \"time\": %.17g}\n", ds.time());
    return 0;
}
