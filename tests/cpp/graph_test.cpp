// graph_test.cpp -- TEST PROGRAM: the graph builder through the C++ mirror
// (abnn::Brain::build_graph) against the rule on the host
// (abnn_graph_fill_host) on a mixed spec: all three topologies, both weight
// laws, block boundaries at 1, 2 and 3 mod 4 and a record count that is no
// multiple of 4; then a refused spec, which must leave the records in place.
//   usage: graph_test   (tests/test_graph_cpp.py; prints one JSON line)
#include <abnn/brain.hpp>

#include <cstdio>
#include <cstring>
#include <vector>

namespace {

int fail(const char* what, long at = -1)
{
    std::printf("{\"ok\": false, \"what\": \"%s\", \"at\": %ld}\n", what, at);
    return 1;
}

abnn_graph_block block(uint64_t count, uint32_t sf, uint32_t sc, uint32_t df, uint32_t dc, uint32_t topo, uint32_t k,
                       float p, uint32_t law, float lo, float hi, uint32_t a, uint32_t b)
{
    abnn_graph_block g;
    std::memset(&g, 0, sizeof(g));
    g.count = count, g.src_first = sf, g.src_count = sc, g.dst_first = df, g.dst_count = dc;
    g.topology = topo, g.k = k, g.p_rewire = p, g.weight_law = law, g.w_lo = lo, g.w_hi = hi;
    g.beta_a = a, g.beta_b = b;
    return g;
}

long first_difference(const std::vector<abnn::SynapsePacked>& got, const std::vector<abnn_synapse>& want)
{
    static_assert(sizeof(abnn::SynapsePacked) == sizeof(abnn_synapse), "the interchange record");
    for (size_t i = 0; i < want.size(); ++i)
        if (std::memcmp(&got[i], &want[i], sizeof(abnn_synapse)) != 0) return (long)i;
    return -1;
}

}  // namespace

int main()
{
    static_assert(sizeof(abnn_graph_block) == 64 && sizeof(abnn_graph_spec) == 1040, "abnn.h graph structs");
    const uint32_t n_in = 16, n_out = 8, n_hid = 4072;  // N_NRN = 4096
    abnn_graph_spec spec;
    std::memset(&spec, 0, sizeof(spec));
    spec.seed = 0x1234567887654321ull;
    spec.n_blocks = 5;
    spec.blocks[0] = block(129, 0, n_in, n_in, n_out, ABNN_TOPO_DENSE, 0, 0.0f, ABNN_W_UNIFORM, 0.4f, 0.8f, 0, 0);
    spec.blocks[1] = block(1, 24, 100, 30, 7, ABNN_TOPO_RANDOM, 0, 0.0f, ABNN_W_BETA, 0.0f, 1.0f, 2, 8);
    spec.blocks[2] = block(40001, 24, n_hid, 24, n_hid, ABNN_TOPO_RANDOM, 0, 0.0f, ABNN_W_UNIFORM, 0.1f, 0.2f, 0, 0);
    spec.blocks[3] = block(30000, 100, 3000, 100, 3000, ABNN_TOPO_RING, 10, 0.1f, ABNN_W_BETA, 0.0f, 0.5f, 2, 8);
    spec.blocks[4] = block(5, 100, 9, 100, 9, ABNN_TOPO_RING, 8, 0.0f, ABNN_W_BETA, -1.0f, 1.0f, 9, 3);
    const uint64_t total = abnn_graph_records(&spec);
    if (total != 129 + 1 + 40001 + 30000 + 5) return fail("abnn_graph_records");

    std::vector<abnn_synapse> want(total);
    abnn::check(abnn_graph_fill_host(&spec, 0, total, want.data()), "abnn_graph_fill_host");

    abnn::Brain a(n_in, n_out, n_hid, (uint32_t)total, 4096);
    a.build_graph(spec);
    std::vector<abnn::SynapsePacked> got(a.n_syn());
    abnn::check(abnn_download_synapses(a.handle(), 0, got.data(), got.size()), "abnn_download_synapses");
    if (got.size() != total) return fail("n_syn");
    long at = first_difference(got, want);
    if (at >= 0) return fail("Brain::build_graph != abnn_graph_fill_host", at);

    // a refusal leaves the records in place: a spec with fewer records than the handle
    abnn_graph_spec small = spec;
    small.blocks[2].count = 40000;
    if (abnn_build_graph(a.handle(), &small) != ABNN_ERR_INVALID) return fail("a short spec was accepted");
    abnn::check(abnn_download_synapses(a.handle(), 0, got.data(), got.size()), "abnn_download_synapses");
    at = first_difference(got, want);
    if (at >= 0) return fail("a refused build changed the records", at);

    const uint64_t checksum = a.checksum();
    std::printf("{\"ok\": true, \"records\": %llu, \"checksum\": %llu}\n", (unsigned long long)total,
                (unsigned long long)checksum);
    return 0;
}
