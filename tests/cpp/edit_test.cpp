// edit_test.cpp -- TEST PROGRAM: the synapse edit through the C++ mirror
// (abnn::Brain::edit, abnn::EditView) against the rule on the host
// (abnn_edit_host) over the generated graph of 100 001 records: every op, a
// weight band with a clamp, both SCALE planes, a draw, and the lesion of the
// 256 outputs' receptive fields.
//   usage: edit_test   (tests/test_edit_gpu.py; prints one JSON line)
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

abnn_edit_config config(uint32_t op)
{
    abnn_edit_config c;
    std::memset(&c, 0, sizeof(c));
    c.op = op;
    return c;
}

std::vector<abnn_synapse> download(abnn::Brain& b)
{
    std::vector<abnn_synapse> s(b.n_syn());
    abnn::check(abnn_download_synapses(b.handle(), 0, s.data(), s.size()), "abnn_download_synapses");
    return s;
}

}  // namespace

int main()
{
    static_assert(sizeof(abnn_edit_config) == 64, "abnn.h abnn_edit_config");
    const uint32_t n_nrn = 1000, n_syn = 100001;
    abnn::Brain a(256, 256, 488, n_syn, 100000);
    a.build_random_graph(1);

    std::vector<float> narrow(256), wide(n_nrn);
    for (size_t i = 0; i < narrow.size(); ++i) narrow[i] = 0.5f + 0.005f * (float)i;
    for (size_t i = 0; i < wide.size(); ++i) wide[i] = 1.5f - 0.001f * (float)i;

    struct Case {
        abnn_edit_config cfg;
        const std::vector<float>* plane;
    };
    std::vector<Case> cases;
    {
        abnn_edit_config c = config(ABNN_EDIT_AFFINE);  // a weight band, clamped
        c.flags = ABNN_EDIT_WEIGHT | ABNN_EDIT_CLAMP;
        c.w_lo = 0.15f, c.w_hi = 0.6f, c.a = 1.25f, c.b = -0.03125f, c.c_lo = 0.2f, c.c_hi = 0.55f;
        cases.push_back({c, nullptr});
        c = config(ABNN_EDIT_SET);  // one projection
        c.src_first = 512, c.src_count = 100, c.b = 0.375f;
        cases.push_back({c, nullptr});
        c = config(ABNN_EDIT_DRAW);
        c.dst_first = 600, c.dst_count = 300, c.a = 0.1f, c.b = 0.2f, c.seed = 0xABCDEF0123456789ull;
        cases.push_back({c, nullptr});
        c = config(ABNN_EDIT_SCALE_DST);
        c.dst_first = 256, c.dst_count = 256;
        cases.push_back({c, &narrow});
        c = config(ABNN_EDIT_SCALE_SRC);
        cases.push_back({c, &wide});
        c = config(ABNN_EDIT_KILL);  // the outputs' receptive fields
        c.dst_first = 256, c.dst_count = 256;
        cases.push_back({c, nullptr});
    }

    uint64_t killed = 0;
    for (size_t k = 0; k < cases.size(); ++k) {
        const Case& cs = cases[k];
        if (abnn_edit_words(&cs.cfg) != ABNN_EDIT_HEADER_WORDS) return fail("abnn_edit_words", (long)k);
        std::vector<abnn_synapse> want = download(a);
        uint64_t head[ABNN_EDIT_HEADER_WORDS];
        abnn::check(abnn_edit_host(&cs.cfg, n_nrn, 0, want.data(), want.size(), cs.plane ? cs.plane->data() : nullptr, head),
                    "abnn_edit_host");
        const std::vector<uint64_t> words = cs.plane ? a.edit(cs.cfg, *cs.plane) : a.edit(cs.cfg);
        if (std::memcmp(words.data(), head, sizeof(head)) != 0) return fail("the header", (long)k);
        const abnn::EditView v(words.data());
        if (v.records() != n_syn || v.matched() == 0 || v.changed() > v.matched()) return fail("EditView", (long)k);
        const std::vector<abnn_synapse> got = download(a);
        for (size_t i = 0; i < want.size(); ++i)
            if (std::memcmp(&got[i], &want[i], sizeof(abnn_synapse)) != 0) return fail("Brain::edit != abnn_edit_host", (long)i);
        killed = v.killed();
    }

    abnn_edit_config bad = config(ABNN_EDIT_KILL);
    bad.flags = ABNN_EDIT_CLAMP;
    uint64_t out[ABNN_EDIT_HEADER_WORDS];
    if (abnn_edit_words(&bad) != 0 || abnn_edit(a.handle(), &bad, nullptr, 0, out) != ABNN_ERR_INVALID)
        return fail("CLAMP with KILL was accepted");

    std::printf("{\"ok\": true, \"records\": %llu, \"killed\": %llu, \"cases\": %zu}\n", (unsigned long long)n_syn,
                (unsigned long long)killed, cases.size());
    return 0;
}
