// corr_test.cpp -- TEST PROGRAM: the spike correlograms through the C++ mirrors
// (abnn::Brain::correlate, abnn::CorrView, Brain::load_spikes) against
// abnn_corr_host: on the raster the recorder took over 16 passes of the
// generated graph, and on a hand-made raster put into the recorder.
//   usage: corr_test   (tests/test_corr_gpu.py; prints one JSON line)
#include <abnn/brain.hpp>

#include <cstdio>
#include <cstdlib>

namespace {

int fail(const char* what, long at = -1)
{
    std::printf("{\"ok\": false, \"what\": \"%s\", \"at\": %ld}\n", what, at);
    return 1;
}

abnn_corr_config config(uint32_t mode, uint32_t af, uint32_t ac, uint32_t bf, uint32_t bc, uint32_t L)
{
    abnn_corr_config c{};
    c.mode = mode;
    c.a_first = af;
    c.a_count = ac;
    c.b_first = bf;
    c.b_count = bc;
    c.max_lag = L;
    return c;
}

}  // namespace

int main()
{
    const uint32_t n_syn = 100000;
    abnn::Brain a(256, 256, 488, n_syn, 100000);
    a.build_random_graph(1);
    a.set_auto_stimulus(0, 256);
    abnn_spikes_config rc{};
    rc.raster_capacity = 1 << 16;
    rc.pass_capacity = 64;
    a.record_spikes(rc);
    a.encode_traversal(nullptr, 16);
    a.synchronize();
    const uint64_t n_nrn = a.n_neuron();
    std::vector<abnn::SynapsePacked> syn(a.n_syn());
    abnn::check(abnn_download_synapses(a.handle(), 0, syn.data(), syn.size()), "abnn_download_synapses");
    std::vector<abnn_spike_pass> passes = a.read_spike_passes();
    std::vector<uint32_t> raster = a.read_spike_raster(0, a.spikes_info().spikes_recorded);
    if (passes.size() != 16 || raster.empty()) return fail("the recorder holds 16 passes");

    abnn_corr_config cfgs[] = {config(ABNN_CORR_POP, 0, 0, 0, 0, 5), config(ABNN_CORR_POP, 512, 488, 256, 256, 16),
                               config(ABNN_CORR_PAIRS, 512, 64, 256, 256, 3), config(ABNN_CORR_SYNAPSES, 0, 0, 0, 0, 5),
                               config(ABNN_CORR_SYNAPSES, 512, 488, 256, 256, 2), config(ABNN_CORR_SYNAPSES, 0, 0, 0, 0, 4)};
    cfgs[5].flags = ABNN_CORR_WEIGHT;
    cfgs[5].w_lo = 0.25f;
    cfgs[5].w_hi = 0.75f;
    cfgs[5].row_first = 3;
    cfgs[5].row_count = 10;
    uint64_t syn_total = 0, followed = 0, coupled = 0, pop0 = 0;
    for (int k = 0; k < 6; ++k) {
        const bool s = cfgs[k].mode == ABNN_CORR_SYNAPSES;
        const std::vector<uint64_t> got = a.correlate(cfgs[k]);
        std::vector<uint64_t> want(abnn_corr_words(&cfgs[k]));
        abnn::check(abnn_corr_host(&cfgs[k], n_nrn, passes.data(), passes.size(), raster.data(), raster.size(),
                                   s ? syn.data() : nullptr, s ? syn.size() : 0, want.data()),
                    "abnn_corr_host");
        if (got != want) return fail("Brain::correlate", k);
        const abnn::CorrView v(got.data(), cfgs[k]);
        if (v.recorded() != 16 || v.rows() != (k == 5 ? 10u : 16u)) return fail("header", k);
        uint64_t sum = 0;
        if (cfgs[k].mode == ABNN_CORR_PAIRS) {
            for (uint32_t x = 512; x < 576; ++x)
                for (uint32_t y = 256; y < 512; ++y)
                    for (int64_t l = -3; l <= 3; ++l) sum += v.at(x, y, l);
        } else {
            for (int64_t l = -(int64_t)cfgs[k].max_lag; l <= (int64_t)cfgs[k].max_lag; ++l) sum += v.at(l);
        }
        if (sum != v.total()) return fail("word 4", k);
        if (k == 0) pop0 = v.at(0);
        if (k == 3) syn_total = v.total(), followed = v.followed(), coupled = v.coupled();
    }
    if (syn_total == 0 || coupled == 0 || followed != n_syn) return fail("the SYNAPSES plane is empty");

    // a hand-made raster through load_spikes: row 0 = 1 1 2, row 1 empty, row 2 = 3, row 3 = 1 999
    const std::vector<uint32_t> r2 = {1, 1, 2, 3, 1, 999};
    const std::vector<abnn_spike_pass> p2 = {{0, 0, 0, 3, 0}, {1, 1, 3, 0, 0}, {2, 2, 3, 1, 0}, {3, 3, 4, 2, 0}};
    a.load_spikes(p2, r2);
    if (a.spikes_info().passes_recorded != 4 || a.read_spike_raster(0, 6) != r2) return fail("load_spikes");
    const abnn_corr_config c = config(ABNN_CORR_PAIRS, 1, 1, 1, 1, 3);
    const std::vector<uint64_t> got = a.correlate(c);
    const std::vector<uint64_t> want = {4, 6, 3, 3, 9, 0, 0, 4, 2, 0, 0, 5, 0, 0, 2};
    if (got != want) return fail("the hand-made raster");
    bool thrown = false;
    try {
        a.load_spikes({{0, 0, 1, 1, 0}}, {5});  // the first offset is not 0
    } catch (const std::runtime_error&) {
        thrown = true;
    }
    if (!thrown || a.spikes_info().passes_recorded != 4) return fail("a bad table was accepted");
    abnn_corr_config bad = c;
    bad.max_lag = 257;
    thrown = false;
    try {
        a.correlate(bad);
    } catch (const std::runtime_error&) {
        thrown = true;
    }
    if (!thrown) return fail("an invalid config was accepted");
    std::printf("{\"ok\": true, \"pop0\": %llu, \"syn_total\": %llu, \"followed\": %llu, \"coupled\": %llu}\n",
                (unsigned long long)pop0, (unsigned long long)syn_total, (unsigned long long)followed,
                (unsigned long long)coupled);
    return 0;
}
