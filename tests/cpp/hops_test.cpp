// hops_test.cpp -- TEST PROGRAM: reachability through the C++ mirrors
// (abnn::Brain::hops, abnn::HopsView) on the generated graph against a host
// breadth-first search over the downloaded records that restates abnn.h's
// steps, and the step path (Brain::hops_step_enqueue) over two handles that
// hold half of the records each, their planes merged on the host between the
// steps.
//   usage: hops_test   (tests/test_hops_gpu.py; prints one JSON line)
#include <abnn/brain.hpp>

#include <dlfcn.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace {

// abnn.h's steps over interchange records
std::vector<uint64_t> host_hops(const std::vector<abnn::SynapsePacked>& syn, const abnn_hops_config& c, uint64_t n_nrn)
{
    const uint32_t H = c.max_hops;
    std::vector<uint64_t> w(abnn_hops_words(&c, n_nrn), 0);
    uint64_t* levels = w.data() + ABNN_HOPS_HEADER_WORDS;
    uint32_t* plane = reinterpret_cast<uint32_t*>(levels + H + 1);
    for (uint64_t n = 0; n < n_nrn; ++n)
        plane[n] = (n >= c.seed_first && n - c.seed_first < c.seed_count) ? 0u : ABNN_HOPS_UNREACHED;
    for (uint32_t h = 0; h <= H; ++h) {
        if (h > 0 && levels[h - 1] == 0) break;
        for (uint64_t n = 0; n < n_nrn; ++n) levels[h] += plane[n] == h;
        if (h == H) break;
        for (const abnn::SynapsePacked& s : syn) {
            if (s.dst == 0xFFFFFFFFu || s.src >= n_nrn || s.dst >= n_nrn) continue;
            if ((c.flags & ABNN_HOPS_WEIGHT) && !(s.w >= c.w_lo && s.w < c.w_hi)) continue;
            const uint32_t u = (c.flags & ABNN_HOPS_REVERSE) ? s.dst : s.src, v = (c.flags & ABNN_HOPS_REVERSE) ? s.src : s.dst;
            if (plane[u] == h) plane[v] = std::min(plane[v], h + 1);
        }
    }
    w[0] = syn.size();
    w[1] = n_nrn;
    for (uint32_t h = 0; h <= H; ++h) {
        w[2] += levels[h];
        if (levels[h]) w[3] = h;
    }
    w[4] = levels[H] == 0;
    return w;
}

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
    std::vector<abnn::SynapsePacked> syn(a.n_syn());
    abnn::check(abnn_download_synapses(a.handle(), 0, syn.data(), syn.size()), "abnn_download_synapses");
    const uint64_t n_nrn = a.n_neuron();

    const abnn_hops_config cfgs[] = {{0, 256, 8, 0, 0.0f, 0.0f, {0, 0}},                       // from the inputs
                                     {256, 256, 8, ABNN_HOPS_REVERSE, 0.0f, 0.0f, {0, 0}},     // who reaches the outputs
                                     {512, 1, 64, 0, 0.0f, 0.0f, {0, 0}},                      // inside the hidden block
                                     {512, 1, 63, ABNN_HOPS_WEIGHT, 0.3f, 0.9f, {0, 0}},
                                     {9999, 1, 1024, ABNN_HOPS_REVERSE | ABNN_HOPS_WEIGHT, 0.3f, 0.9f, {0, 0}},
                                     {600, 40, 2, 0, 0.0f, 0.0f, {0, 0}}};                     // cut off by H
    uint64_t hidden_reached = 0, hidden_depth = 0, in_l0 = 0, in_l1 = 0, cut_complete = 1;
    for (int k = 0; k < 6; ++k) {
        const std::vector<uint64_t> got = a.hops(cfgs[k]), want = host_hops(syn, cfgs[k], n_nrn);
        if (got != want) return fail("Brain::hops", k);
        const abnn::HopsView v(got.data(), cfgs[k]);
        if (v.records() != n_syn || v.neurons() != n_nrn) return fail("header", k);
        uint64_t sum = 0, at_depth = 0, reached = 0;
        for (uint32_t h = 0; h <= cfgs[k].max_hops; ++h) sum += v.levels()[h];
        for (uint64_t n = 0; n < n_nrn; ++n) {
            reached += v.dist()[n] != ABNN_HOPS_UNREACHED;
            at_depth += v.dist()[n] == v.depth();
        }
        if (sum != v.reached() || reached != v.reached() || at_depth != v.levels()[v.depth()]) return fail("invariant", k);
        if (v.complete() != (v.levels()[cfgs[k].max_hops] == 0)) return fail("complete", k);
        if (k == 0) in_l0 = v.levels()[0], in_l1 = v.levels()[1];
        if (k == 2) hidden_reached = v.reached(), hidden_depth = v.depth();
        if (k == 5) cut_complete = v.complete();
    }

    abnn_hops_config bad = cfgs[0];
    bad.seed_count = 0;
    bool thrown = false;
    try {
        a.hops(bad);
    } catch (const std::runtime_error&) {
        thrown = true;
    }
    if (!thrown) return fail("an invalid config was accepted");

    // the step path: two handles with half of the records each
    auto hipMalloc = hip<int (*)(void**, size_t)>("hipMalloc");
    auto hipFree = hip<int (*)(void*)>("hipFree");
    auto hipMemcpy = hip<int (*)(void*, const void*, size_t, int)>("hipMemcpy");  // kind 1: to the device, 2: from it
    const abnn_hops_config& c = cfgs[2];
    const std::vector<uint64_t> whole = a.hops(c);
    const uint64_t words = whole.size(), half = n_syn / 2 + 1, at = ABNN_HOPS_HEADER_WORDS + c.max_hops + 1;
    abnn::Brain s0(256, 256, 9488, (uint32_t)half, 100000), s1(256, 256, 9488, (uint32_t)(n_syn - half), 100000);
    abnn::check(abnn_upload_synapses(s0.handle(), 0, syn.data(), half), "abnn_upload_synapses");
    abnn::check(abnn_upload_synapses(s1.handle(), 0, syn.data() + half, n_syn - half), "abnn_upload_synapses");
    abnn::Brain* shard[2] = {&s0, &s1};
    uint64_t* dev[2] = {nullptr, nullptr};
    std::vector<uint64_t> part[2] = {std::vector<uint64_t>(words), std::vector<uint64_t>(words)};
    for (int r = 0; r < 2; ++r) {
        if (hipMalloc(reinterpret_cast<void**>(&dev[r]), words * 8) != 0) return fail("hipMalloc", r);
        shard[r]->hops_step_enqueue(c, ABNN_HOPS_BEGIN, dev[r]);
    }
    for (uint32_t h = 0; h <= c.max_hops; ++h) {
        for (int r = 0; r < 2; ++r) shard[r]->hops_step_enqueue(c, h, dev[r]);
        if (h == c.max_hops) break;
        // hipMemcpy on the null stream follows the step's kernels
        for (int r = 0; r < 2; ++r)
            if (hipMemcpy(part[r].data() + at, dev[r] + at, (words - at) * 8, 2) != 0) return fail("hipMemcpy", r);
        uint32_t* p0 = reinterpret_cast<uint32_t*>(part[0].data() + at);
        const uint32_t* p1 = reinterpret_cast<const uint32_t*>(part[1].data() + at);
        for (uint64_t n = 0; n < n_nrn; ++n) p0[n] = std::min(p0[n], p1[n]);
        for (int r = 0; r < 2; ++r)
            if (hipMemcpy(dev[r] + at, part[0].data() + at, (words - at) * 8, 1) != 0) return fail("hipMemcpy", r);
    }
    bool refused = false;
    try {
        s0.hops_step_enqueue(c, c.max_hops + 1, dev[0]);  // refused on the host: nothing is launched
    } catch (const std::runtime_error&) {
        refused = true;
    }
    if (!refused) return fail("an invalid step was accepted");
    for (int r = 0; r < 2; ++r) {
        if (hipMemcpy(part[r].data(), dev[r], words * 8, 2) != 0) return fail("hipMemcpy", r);
        (void)hipFree(dev[r]);
        if (part[r][0] != (r ? n_syn - half : half)) return fail("a shard's word 0", r);
        part[r][0] = whole[0];
        if (part[r] != whole) return fail("the step path", r);
    }
    std::printf("{\"ok\": true, \"records\": %llu, \"neurons\": %llu, \"inputs_level0\": %llu, \"inputs_level1\": %llu, "
                "\"hidden_reached\": %llu, \"hidden_depth\": %llu, \"cut_complete\": %llu}\n",
                (unsigned long long)n_syn, (unsigned long long)n_nrn, (unsigned long long)in_l0, (unsigned long long)in_l1,
                (unsigned long long)hidden_reached, (unsigned long long)hidden_depth, (unsigned long long)cut_complete);
    return 0;
}
