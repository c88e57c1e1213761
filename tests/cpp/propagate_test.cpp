// propagate_test.cpp -- TEST PROGRAM: signal propagation through the C++
// mirrors (abnn::Brain::propagate / branching, abnn::PropagateView) on the
// generated graph against the library's host rule (abnn_propagate_host) over
// the downloaded records, and the enqueue-only iteration
// (Brain::propagate_iterate_enqueue) on device planes against Brain::branching.
//   usage: propagate_test   (tests/test_propagate_gpu.py; prints one JSON line)
#include <abnn/brain.hpp>

#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>

namespace {

int fail(const char* what, long at = -1)
{
    std::printf("{\"ok\": false, \"what\": \"%s\", \"at\": %ld}\n", what, at);
    return 1;
}

// The HIP runtime is in the process through the library: device memory for the
// enqueue-only path without a compile-time dependency on it.
template <class F>
F hip(const char* name)
{
    void* p = dlsym(RTLD_DEFAULT, name);
    if (!p) {
        fail(name);
        std::exit(1);
    }
    return reinterpret_cast<F>(p);
}

}  // namespace

int main()
{
    const uint32_t n_syn = 100000;
    abnn::Brain a(256, 256, 9488, n_syn, 100000);
    a.build_random_graph(1);
    std::vector<abnn_synapse> syn(a.n_syn());
    abnn::check(abnn_download_synapses(a.handle(), 0, syn.data(), syn.size()), "abnn_download_synapses");
    const uint64_t n_nrn = a.n_neuron();
    abnn_params params{};
    abnn::check(abnn_get_params(a.handle(), &params), "abnn_get_params");

    // a seeded plane: one neuron in three silent, both signs
    std::vector<int32_t> x(n_nrn);
    uint64_t s = 12345;
    for (uint64_t n = 0; n < n_nrn; ++n) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        x[n] = (s >> 61) < 3 ? 0 : (int32_t)(s >> 32);
    }
    std::vector<int32_t> hot(n_nrn, 0);
    hot[3] = 1 << 30;

    const abnn_propagate_config cfgs[] = {
        {0, 0, 0, 0, 0, 0.0f, 0.0f, {0, 0, 0, 0, 0}},                                          // W x over every neuron
        {0, 0, 0, 0, ABNN_PROP_REVERSE | ABNN_PROP_FIRE_P, 0.0f, 0.0f, {0, 0, 0, 0, 0}},       // the transpose, fire probabilities
        {0, 256, 256, 256, 0, 0.0f, 0.0f, {0, 0, 0, 0, 0}},                                    // inputs -> outputs: a narrow out-range
        {512, 9488, 512, 9488, ABNN_PROP_WEIGHT | ABNN_PROP_FIRE_P, 0.3f, 0.9f, {0, 0, 0, 0, 0}}};  // the hidden block, a weight band
    uint64_t followed0 = 0, outputs_followed = 0;
    for (int k = 0; k < 4; ++k) {
        for (int h = 0; h < 2; ++h) {
            const std::vector<int32_t>& xin = h ? hot : x;
            const std::vector<uint64_t> got = a.propagate(cfgs[k], xin);
            std::vector<uint64_t> want(abnn_propagate_words(&cfgs[k], n_nrn));
            abnn::check(abnn_propagate_host(&cfgs[k], n_nrn, params.base_scale, syn.data(), syn.size(), xin.data(), want.data()),
                        "abnn_propagate_host");
            if (got != want) return fail("Brain::propagate", 2 * k + h);
            const abnn::PropagateView v(got.data(), cfgs[k], n_nrn);
            if (v.records() != n_syn || v.tombstones() != 0 || v.followed() > v.records() || v.skipped() != 0)
                return fail("header", 2 * k + h);
            if (v.count != (cfgs[k].out_count ? cfgs[k].out_count : n_nrn)) return fail("count", k);
            bool any = false;
            for (uint64_t j = 0; j < v.count; ++j) any |= v.y()[j] != 0;
            if (any != (v.followed() != 0)) return fail("y against followed", 2 * k + h);
            if (k == 0 && h == 0) followed0 = v.followed();
            if (k == 2 && h == 1) outputs_followed = v.followed();
        }
    }

    abnn_propagate_config bad = cfgs[0];
    bad.flags = 8;
    bool thrown = false;
    try {
        a.propagate(bad, x);
    } catch (const std::runtime_error&) {
        thrown = true;
    }
    if (!thrown) return fail("an invalid config was accepted");

    // the branching ratio of the hidden block, stepped through the host and enqueued on device planes
    const abnn_propagate_config hid = {512, 9488, 512, 9488, ABNN_PROP_FIRE_P, 0.0f, 0.0f, {0, 0, 0, 0, 0}};
    const uint32_t steps = 6;
    std::vector<int32_t> x0(n_nrn, 0);
    for (uint64_t n = 512; n < n_nrn; ++n) x0[n] = 1 << 29;
    const abnn::Branching br = a.branching(hid, steps, x0);
    if (br.steps() != steps || !(br.ratio() > 0.0)) return fail("Brain::branching");

    auto hipMalloc = hip<int (*)(void**, size_t)>("hipMalloc");
    auto hipFree = hip<int (*)(void*)>("hipFree");
    auto hipMemcpy = hip<int (*)(void*, const void*, size_t, int)>("hipMemcpy");  // kind 1: to the device, 2: from it
    const uint64_t words = abnn_propagate_words(&hid, n_nrn);
    int32_t* x_dev = nullptr;
    uint64_t *work_dev = nullptr, *trace_dev = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&x_dev), n_nrn * 4) != 0 || hipMalloc(reinterpret_cast<void**>(&work_dev), words * 8) != 0 ||
        hipMalloc(reinterpret_cast<void**>(&trace_dev), steps * ABNN_PROP_TRACE_WORDS * 8) != 0)
        return fail("hipMalloc");
    if (hipMemcpy(x_dev, x0.data(), n_nrn * 4, 1) != 0) return fail("hipMemcpy");
    a.propagate_iterate_enqueue(hid, steps, x_dev, work_dev, trace_dev);
    std::vector<uint64_t> trace(steps * ABNN_PROP_TRACE_WORDS);
    std::vector<int32_t> x_end(n_nrn);
    // hipMemcpy on the null stream follows the iteration's kernels
    if (hipMemcpy(trace.data(), trace_dev, trace.size() * 8, 2) != 0 || hipMemcpy(x_end.data(), x_dev, n_nrn * 4, 2) != 0)
        return fail("hipMemcpy");
    if (trace != br.trace) return fail("the enqueued iteration's trace");
    if (x_end != br.x) return fail("the enqueued iteration's plane");
    bool refused = false;
    try {
        a.propagate_iterate_enqueue(cfgs[2], steps, x_dev, work_dev, trace_dev);  // in-range != out-range
    } catch (const std::runtime_error&) {
        refused = true;
    }
    if (!refused) return fail("an iteration over unequal ranges was accepted");
    (void)hipFree(x_dev);
    (void)hipFree(work_dev);
    (void)hipFree(trace_dev);

    std::printf("{\"ok\": true, \"records\": %llu, \"neurons\": %llu, \"followed\": %llu, \"outputs_followed\": %llu, "
                "\"steps\": %u, \"ratio\": %.9g}\n",
                (unsigned long long)n_syn, (unsigned long long)n_nrn, (unsigned long long)followed0,
                (unsigned long long)outputs_followed, steps, br.ratio());
    return 0;
}
