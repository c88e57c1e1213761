// select_test.cpp -- TEST PROGRAM: the synapse select through the C++ mirrors
// (abnn::Brain::select, abnn::SelectView) on the generated graph against a host
// loop over the downloaded records that restates abnn.h's matching rule: ALL
// and ANY, with and without a weight bound, capacities below, at and above the
// matches.
//   usage: select_test   (tests/test_select_gpu.py; prints one JSON line)
#include <abnn/brain.hpp>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

namespace {

bool host_match(const abnn::SynapsePacked& s, const abnn_select_config& c)
{
    if (s.dst == 0xFFFFFFFFu) return false;
    const bool S = (uint32_t)(s.src - c.src_first) < c.src_count, D = (uint32_t)(s.dst - c.dst_first) < c.dst_count;
    bool m;
    if (c.flags & ABNN_SELECT_ANY)
        m = S || D;
    else
        m = (S || !c.src_count) && (D || !c.dst_count);
    if (c.flags & ABNN_SELECT_WEIGHT) m = m && s.w >= c.w_lo && s.w < c.w_hi;
    return m;
}

// abnn.h's select over interchange records, one record at a time
std::vector<uint64_t> host_select(const std::vector<abnn::SynapsePacked>& syn, const abnn_select_config& c,
                                  uint64_t capacity)
{
    std::vector<uint64_t> w(abnn_select_words(&c, capacity), 0);
    abnn_synapse* rec = reinterpret_cast<abnn_synapse*>(w.data() + ABNN_SELECT_HEADER_WORDS + capacity);
    w[0] = syn.size();
    for (uint64_t i = 0; i < syn.size(); ++i) {
        if (syn[i].dst == 0xFFFFFFFFu) w[1] += 1;
        if (!host_match(syn[i], c)) continue;
        if (w[2] < capacity) {
            w[ABNN_SELECT_HEADER_WORDS + w[2]] = i;
            rec[w[2]] = abnn_synapse{syn[i].src, syn[i].dst, syn[i].w, 0.0f};
        }
        w[2] += 1;
    }
    w[3] = std::min<uint64_t>(w[2], capacity);
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
    const uint32_t n_syn = 100001;  // the last record is in no 16-byte pair
    abnn::Brain a(256, 256, 9488, n_syn, 100000);
    a.build_random_graph(1);
    std::vector<abnn::SynapsePacked> syn(a.n_syn());
    abnn::check(abnn_download_synapses(a.handle(), 0, syn.data(), syn.size()), "abnn_download_synapses");

    const float inf = std::numeric_limits<float>::infinity();
    const abnn_select_config cfgs[] = {
        {0, 0, 256, 256, 0.0f, 0.0f, 0, 0},                                        // the outputs' receptive fields
        {0, 256, 0, 0, 0.0f, 0.0f, 0, 0},                                          // what leaves the inputs
        {512, 1000, 512, 1000, 0.0f, 0.0f, ABNN_SELECT_ANY, 0},                    // a hidden window's neighbourhood
        {512, 1000, 512, 1000, 0.0f, 0.0f, 0, 0},                                  // its induced subgraph
        {0, 0, 0, 0, 0.19f, inf, ABNN_SELECT_WEIGHT, 0},                           // at least 0.19
        {0, 0, 0, 0, 0.0f, 0.0f, 0, 0},                                            // every record
        {0, 16, 256, 256, 0.5f, 0.7f, ABNN_SELECT_WEIGHT, 0},                      // all three
    };
    uint64_t fields = 0, everything = 0;
    for (int k = 0; k < 7; ++k) {
        const uint64_t matched = abnn::SelectView(a.select(cfgs[k], 0).data(), 0).matched();
        const uint64_t caps[] = {0, 1, matched ? matched - 1 : 0, matched, matched + 1};
        for (uint64_t cap : caps) {
            const std::vector<uint64_t> got = a.select(cfgs[k], cap), want = host_select(syn, cfgs[k], cap);
            if (got != want) return fail("Brain::select", k);
            const abnn::SelectView v(got.data(), cap);
            if (v.records() != n_syn || v.tombstones() != 0 || v.matched() != matched ||
                v.written() != std::min(matched, cap) || v.syn_offset() != 0)
                return fail("header", k);
            for (uint64_t j = 0; j < v.written(); ++j) {
                const abnn::SynapsePacked& s = syn[v.index()[j]];
                if (std::memcmp(&s.src, &v.syn()[j].src, 12) != 0 || (j && v.index()[j] <= v.index()[j - 1]))
                    return fail("SelectView", k);
            }
        }
        if (k == 0) fields = matched;
        if (k == 5) everything = matched;
    }
    if (fields != 65536 || everything != n_syn) return fail("the generated graph's counts");

    abnn_select_config bad = cfgs[0];
    bad.flags = ABNN_SELECT_ANY;
    bad.dst_count = 0;  // ANY with no range set
    bool thrown = false;
    try {
        a.select(bad, 4);
    } catch (const std::runtime_error&) {
        thrown = true;
    }
    if (!thrown) return fail("an invalid config was accepted");

    std::printf("{\"ok\": true, \"records\": %llu, \"receptive_fields\": %llu, \"everything\": %llu}\n",
                (unsigned long long)n_syn, (unsigned long long)fields, (unsigned long long)everything);
    return 0;
}
