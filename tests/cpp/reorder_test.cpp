// reorder_test.cpp -- TEST PROGRAM: the record reorder through the C++ mirror
// (abnn::Brain::reorder, abnn::ReorderView) against the rule on the host
// (abnn_reorder_host) over the generated graph of 100 001 records with a few
// tombstones: every key, both directions, a shuffle, the compaction, and a
// reorder undone by PERM with the inverse of its origin.
//   usage: reorder_test   (tests/test_reorder_gpu.py; prints one JSON line)
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

abnn_reorder_config config(uint32_t key, uint32_t flags, uint64_t seed = 0)
{
    abnn_reorder_config c;
    std::memset(&c, 0, sizeof(c));
    c.key = key, c.flags = flags, c.seed = seed;
    return c;
}

std::vector<abnn_synapse> download(abnn::Brain& b)
{
    std::vector<abnn_synapse> s(b.n_syn());
    abnn::check(abnn_download_synapses(b.handle(), 0, s.data(), s.size()), "abnn_download_synapses");
    return s;
}

bool same(const std::vector<abnn_synapse>& a, const std::vector<abnn_synapse>& b, long* at)
{
    for (size_t i = 0; i < a.size(); ++i)
        if (std::memcmp(&a[i], &b[i], sizeof(abnn_synapse)) != 0) {
            *at = (long)i;
            return false;
        }
    return a.size() == b.size();
}

}  // namespace

int main()
{
    static_assert(sizeof(abnn_reorder_config) == 32, "abnn.h abnn_reorder_config");
    const uint32_t n_syn = 100001;
    abnn::Brain a(256, 256, 488, n_syn, 100000);
    a.build_random_graph(1);
    {  // tombstones at the first, the last and scattered indices
        std::vector<abnn_synapse> s = download(a);
        for (size_t i : {(size_t)0, (size_t)4095, (size_t)4096, (size_t)50000, (size_t)n_syn - 1})
            s[i].src = s[i].dst = 0xFFFFFFFFu;
        abnn::check(abnn_upload_synapses(a.handle(), 0, s.data(), s.size()), "abnn_upload_synapses");
    }
    const std::vector<abnn_synapse> first = download(a);

    const abnn_reorder_config cases[] = {
        config(ABNN_REORDER_DST, ABNN_REORDER_ORIGIN),
        config(ABNN_REORDER_SRC, ABNN_REORDER_ORIGIN | ABNN_REORDER_DESCENDING),
        config(ABNN_REORDER_W, ABNN_REORDER_ORIGIN),
        config(ABNN_REORDER_W, ABNN_REORDER_DESCENDING),
        config(ABNN_REORDER_RANDOM, ABNN_REORDER_ORIGIN, 0xABCDEF0123456789ull),
        config(ABNN_REORDER_NONE, ABNN_REORDER_ORIGIN),
        config(ABNN_REORDER_SRC, 0),
    };
    uint64_t moved = 0;
    long at = -1;
    size_t k = 0;
    for (const abnn_reorder_config& cfg : cases) {
        const uint64_t words = abnn_reorder_words(&cfg, n_syn);
        if (words != 8 + ((cfg.flags & ABNN_REORDER_ORIGIN) ? (n_syn + 1) / 2 : 0)) return fail("abnn_reorder_words", (long)k);
        std::vector<abnn_synapse> want = download(a);
        std::vector<uint64_t> head(words);
        abnn::check(abnn_reorder_host(&cfg, 0, want.data(), want.size(), nullptr, head.data()), "abnn_reorder_host");
        const std::vector<uint64_t> got = a.reorder(cfg);
        if (got.size() != words || std::memcmp(got.data(), head.data(), words * 8) != 0) return fail("the result's words", (long)k);
        const abnn::ReorderView v(got.data());
        if (v.records() != n_syn || v.tombstones() != 5 || v.invalid() != 0) return fail("ReorderView", (long)k);
        if (!same(download(a), want, &at)) return fail("Brain::reorder != abnn_reorder_host", at);
        moved += v.moved();
        ++k;
    }

    // a reorder by dst, undone by PERM with the inverse of its origin
    abnn::check(abnn_upload_synapses(a.handle(), 0, first.data(), first.size()), "abnn_upload_synapses");
    const std::vector<uint64_t> by_dst = a.reorder(config(ABNN_REORDER_DST, ABNN_REORDER_ORIGIN));
    const abnn::ReorderView v(by_dst.data());
    std::vector<uint32_t> inverse(n_syn);
    for (uint32_t i = 0; i < n_syn; ++i) inverse[v.origin()[i]] = i;
    const std::vector<uint64_t> back = a.reorder(config(ABNN_REORDER_PERM, 0), inverse);
    if (abnn::ReorderView(back.data()).invalid() != 0 || abnn::ReorderView(back.data()).moved() != v.moved())
        return fail("PERM with the inverse");
    if (!same(download(a), first, &at)) return fail("PERM did not undo the reorder", at);
    inverse[7] = inverse[8];  // a repeat: nothing moves
    const std::vector<uint64_t> refused = a.reorder(config(ABNN_REORDER_PERM, 0), inverse);
    if (abnn::ReorderView(refused.data()).invalid() != 1 || abnn::ReorderView(refused.data()).moved() != 0)
        return fail("an invalid perm was not counted");
    if (!same(download(a), first, &at)) return fail("an invalid perm moved records", at);

    abnn_reorder_config bad = config(ABNN_REORDER_NONE, ABNN_REORDER_DESCENDING);
    uint64_t out[ABNN_REORDER_HEADER_WORDS];
    if (abnn_reorder_words(&bad, n_syn) != 0 || abnn_reorder(a.handle(), &bad, nullptr, out, 8) != ABNN_ERR_INVALID)
        return fail("DESCENDING with NONE was accepted");

    std::printf("{\"ok\": true, \"records\": %llu, \"moved\": %llu, \"cases\": %zu}\n", (unsigned long long)n_syn,
                (unsigned long long)moved, k);
    return 0;
}
