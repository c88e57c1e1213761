// components_test.cpp -- TEST PROGRAM: connected components through the C++
// mirrors (abnn::Brain::components, abnn::ComponentsView) on the generated graph
// against abnn_components_host over the downloaded records, for every flag
// combination, a sub-range and a weight threshold that fragments the graph.
//   usage: components_test   (tests/test_components_gpu.py; prints one JSON line)
#include <abnn/brain.hpp>

#include <cmath>
#include <cstdio>

namespace {

int fail(const char* what, long at = -1)
{
    std::printf("{\"ok\": false, \"what\": \"%s\", \"at\": %ld}\n", what, at);
    return 1;
}

}  // namespace

int main()
{
    const uint32_t n_syn = 100000;
    abnn::Brain a(256, 256, 9488, n_syn, 100000);
    a.build_random_graph(1);
    std::vector<abnn::SynapsePacked> syn(a.n_syn());
    abnn::check(abnn_download_synapses(a.handle(), 0, syn.data(), syn.size()), "abnn_download_synapses");
    const uint64_t n_nrn = a.n_neuron();
    const uint32_t N = (uint32_t)n_nrn;

    const abnn_components_config cfgs[] = {
        {0, N, 0, 0.0f, 0.0f, {0, 0, 0}},                                             // the whole network
        {0, N, ABNN_COMP_SIZES, 0.0f, 0.0f, {0, 0, 0}},                               // ... with the size plane
        {0, N, ABNN_COMP_WEIGHT | ABNN_COMP_SIZES, 0.6f, INFINITY, {0, 0, 0}},        // a threshold that fragments it
        {512, N - 512, ABNN_COMP_WEIGHT, 0.0f, 0.5f, {0, 0, 0}},                      // the hidden block alone
        {0, 512, ABNN_COMP_SIZES, 0.0f, 0.0f, {0, 0, 0}},                             // inputs and outputs: the dense block
    };
    uint64_t whole_components = 0, whole_largest = 0, cut_components = 0, io_largest = 0;
    long k = 0;
    for (const abnn_components_config& c : cfgs) {
        const std::vector<uint64_t> got = a.components(c);
        std::vector<uint64_t> want(abnn_components_words(&c, n_nrn));
        if (got.size() != want.size()) return fail("words", k);
        abnn::check(abnn_components_host(syn.data(), syn.size(), &c, n_nrn, want.data(), want.size()), "abnn_components_host");
        for (size_t j = 0; j < want.size(); ++j)
            if (got[j] != want[j]) return fail("a word differs from abnn_components_host", (long)j);
        const abnn::ComponentsView v(got.data(), c);
        if (v.records() != syn.size() || v.neurons() != n_nrn || v.gave_up() != 0) return fail("header", k);
        uint64_t in_range = 0, largest_members = 0, bins = 0;
        for (uint64_t n = 0; n < n_nrn; ++n) {
            const bool in = n >= c.first && n - c.first < c.count;
            if (in != (v.labels()[n] != ABNN_COMP_NONE)) return fail("NONE outside the range", (long)n);
            if (!in) continue;
            in_range += 1;
            if (v.labels()[n] > n || v.labels()[v.labels()[n]] != v.labels()[n]) return fail("a label is no smallest id", (long)n);
            largest_members += v.labels()[n] == v.largest_label();
            if (v.sizes() && v.sizes()[n] != v.sizes()[v.labels()[n]]) return fail("sizes", (long)n);
        }
        for (uint32_t j = 0; j < ABNN_COMP_SIZE_BINS; ++j) bins += v.bins()[j];
        if (largest_members != v.largest() || bins != v.components() || v.bins()[0] != v.singletons()) return fail("counts", k);
        if ((v.sizes() != nullptr) != ((c.flags & ABNN_COMP_SIZES) != 0)) return fail("sizes view", k);
        if (k == 0) whole_components = v.components(), whole_largest = v.largest();
        if (k == 2) cut_components = v.components();
        if (k == 4) io_largest = v.largest();
        k += 1;
    }
    std::printf("{\"ok\": true, \"records\": %llu, \"neurons\": %llu, \"whole_components\": %llu, \"whole_largest\": %llu, "
                "\"cut_components\": %llu, \"io_largest\": %llu}\n",
                (unsigned long long)syn.size(), (unsigned long long)n_nrn, (unsigned long long)whole_components,
                (unsigned long long)whole_largest, (unsigned long long)cut_components, (unsigned long long)io_largest);
    return 0;
}
