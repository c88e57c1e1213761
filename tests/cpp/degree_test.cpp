// degree_test.cpp -- TEST PROGRAM: the neuron degree census through the C++
// mirrors (abnn::Brain::degrees, abnn::DegreeView) on the generated graph
// against a host loop over the downloaded records that restates abnn.h's
// definition: every neuron (the wide path) and three ranges (the narrow path).
//   usage: degree_test   (tests/test_degree_gpu.py; prints one JSON line)
#include <abnn/brain.hpp>

#include <cmath>
#include <cstdio>

namespace {

// abnn.h's degree census over interchange records, one record at a time
std::vector<uint64_t> host_degrees(const std::vector<abnn::SynapsePacked>& syn, const abnn_degree_config& c,
                                   uint64_t n_nrn)
{
    const uint64_t m = c.count ? c.count : n_nrn, first = c.count ? c.first : 0;
    std::vector<uint64_t> w(abnn_degree_words(&c, n_nrn), 0);
    uint64_t* plane[4] = {nullptr, nullptr, nullptr, nullptr};  // OUT, IN, OUT_W, IN_W
    uint64_t at = ABNN_DEGREE_HEADER_WORDS;
    for (int k = 0; k < 4; ++k)
        if (c.what & (1u << k)) {
            plane[k] = w.data() + at;
            at += m;
        }
    w[0] = syn.size();
    for (const abnn::SynapsePacked& s : syn) {
        if (s.dst == 0xFFFFFFFFu) {
            w[1] += 1;
            continue;
        }
        const bool ok = std::fabs(s.w) < 128.0f;
        const uint64_t q = ok ? (uint64_t)(int64_t)(int32_t)(s.w * 16777216.0f) : 0;
        const uint32_t key[2] = {s.src, s.dst};
        for (int d = 0; d < 2; ++d) {
            if (!(plane[d] || plane[d + 2]) || key[d] < first || key[d] - first >= m) continue;
            w[2 + d] += 1;
            if (plane[d]) plane[d][key[d] - first] += 1;
            if (plane[d + 2]) {
                plane[d + 2][key[d] - first] += q;  // modulo 2^64
                w[4 + d] += ok ? 0 : 1;
            }
        }
    }
    return w;
}

int fail(const char* what, long at = -1)
{
    std::printf("{\"ok\": false, \"what\": \"%s\", \"at\": %ld}\n", what, at);
    return 1;
}

}  // namespace

int main()
{
    const uint32_t n_syn = 100000;
    abnn::Brain a(256, 256, 9488, n_syn, 100000);  // 10 000 neurons: every neuron is a wide range
    a.build_random_graph(1);
    std::vector<abnn::SynapsePacked> syn(a.n_syn());
    abnn::check(abnn_download_synapses(a.handle(), 0, syn.data(), syn.size()), "abnn_download_synapses");
    const uint64_t n_nrn = a.n_neuron();

    const abnn_degree_config cfgs[] = {{0, 0, 15, {0, 0, 0, 0, 0}},
                                       {256, 256, ABNN_DEG_IN | ABNN_DEG_IN_W, {0, 0, 0, 0, 0}},
                                       {0, 256, ABNN_DEG_OUT | ABNN_DEG_OUT_W, {0, 0, 0, 0, 0}},
                                       {512, 4096, 15, {0, 0, 0, 0, 0}},
                                       {9999, 1, ABNN_DEG_IN_W, {0, 0, 0, 0, 0}}};
    uint64_t out_total = 0, min_out_in = ~0ull, max_out_in = 0, min_in_out = ~0ull, max_in_out = 0;
    double in_w_lo = 1e30, in_w_hi = -1e30;
    for (int k = 0; k < 5; ++k) {
        const std::vector<uint64_t> got = a.degrees(cfgs[k]), want = host_degrees(syn, cfgs[k], n_nrn);
        if (got != want) return fail("Brain::degrees", k);
        const abnn::DegreeView v(got.data(), cfgs[k], n_nrn);
        uint64_t so = 0, si = 0;
        for (uint64_t j = 0; j < v.count; ++j) {
            so += v.out() ? v.out()[j] : 0;
            si += v.in() ? v.in()[j] : 0;
        }
        if ((v.out() && so != v.out_total()) || (v.in() && si != v.in_total())) return fail("invariant", k);
        if (v.records() != n_syn || v.tombstones() != 0) return fail("header", k);
        if (k == 0) out_total = v.out_total();
        if (k == 1)  // the outputs: 256 inputs each, weights in [0.4, 0.8)
            for (uint64_t j = 0; j < v.count; ++j) {
                min_out_in = std::min(min_out_in, v.in()[j]);
                max_out_in = std::max(max_out_in, v.in()[j]);
                in_w_lo = std::min(in_w_lo, (double)v.in_w()[j] / 16777216.0);
                in_w_hi = std::max(in_w_hi, (double)v.in_w()[j] / 16777216.0);
            }
        if (k == 2)  // the inputs: 256 outputs each
            for (uint64_t j = 0; j < v.count; ++j) {
                min_in_out = std::min(min_in_out, v.out()[j]);
                max_in_out = std::max(max_in_out, v.out()[j]);
            }
    }
    if (out_total != n_syn) return fail("out_total");
    if (min_out_in != 256 || max_out_in != 256 || min_in_out != 256 || max_in_out != 256) return fail("dense block");
    if (!(in_w_lo >= 256 * 0.4 && in_w_hi < 256 * 0.8)) return fail("in_w of the outputs");

    abnn_degree_config bad = cfgs[0];
    bad.first = 1;  // count 0 with first != 0
    bool thrown = false;
    try {
        a.degrees(bad);
    } catch (const std::runtime_error&) {
        thrown = true;
    }
    if (!thrown) return fail("an invalid config was accepted");

    std::printf("{\"ok\": true, \"records\": %llu, \"neurons\": %llu, \"out_total\": %llu, \"in_degree_of_outputs\": %llu}\n",
                (unsigned long long)n_syn, (unsigned long long)n_nrn, (unsigned long long)out_total,
                (unsigned long long)max_out_in);
    return 0;
}
