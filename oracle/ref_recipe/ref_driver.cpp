// ref_driver.cpp -- the reference's RateFilter (core/output-filter/
// rate-filter.h) and FunctionalDataset (stimulus/functional-dataset.cpp),
// compiled in place and run over the grid of tests/cpp/driver_grid.hpp.
// TEST INFRASTRUCTURE ONLY: built by abnn_amd/build.py: build_reference() into
// oracle/_ref/ (never committed).  The reference's files are included by name
// through -I <checkout>/abnn/src; stub/brain-engine.h stands in for the one
// header of theirs that needs the Metal host API.
#include <cmath>

#include "core/output-filter/rate-filter.h"
#include "stimulus/functional-dataset.cpp"

#include "driver_grid.hpp"

// The functions the reference's app wires in (view-delegate.cpp:37-42).
static float cos_squared(float x) { return std::cos(x) * std::cos(x); }
static float half_sine(float x) { return 0.5f * std::sin(x) + 0.5f; }

int main()
{
    driver_grid::print_all<RateFilter, FunctionalDataset>(&cos_squared, &half_sine);
    return 0;
}
