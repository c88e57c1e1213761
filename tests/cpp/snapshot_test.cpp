// snapshot_test.cpp -- TEST PROGRAM: device-side snapshots through the C++
// mirror (abnn::Brain::snapshot / restore / diff, abnn::Snapshot,
// abnn::DiffView) on the generated graph of 100 001 records: the diff after
// learning passes against the rule on the host (abnn_snapshot_diff_host) over
// the two downloads, a diff of two snapshots, and restore-then-run against the
// run straight after the capture.
//   usage: snapshot_test   (tests/test_snapshot_gpu.py; prints one JSON line)
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

std::vector<abnn_synapse> download(abnn::Brain& b)
{
    std::vector<abnn_synapse> s(b.n_syn());
    abnn::check(abnn_download_synapses(b.handle(), 0, s.data(), s.size()), "abnn_download_synapses");
    return s;
}

bool same(const std::vector<abnn_synapse>& a, const std::vector<abnn_synapse>& b)
{
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(abnn_synapse)) == 0;
}

bool same(const abnn_scalars& a, const abnn_scalars& b)
{
    return a.clock == b.clock && a.pass_index == b.pass_index && std::memcmp(&a.reward, &b.reward, 4) == 0 &&
           std::memcmp(&a.rbar, &b.rbar, 4) == 0;
}

}  // namespace

int main()
{
    static_assert(sizeof(abnn_diff_config) == 32, "abnn.h abnn_diff_config");
    const uint32_t n_nrn = 1000, n_syn = 100001;
    abnn::Brain a(256, 256, 488, n_syn, 100000);
    a.build_random_graph(1);
    a.set_auto_stimulus(0, 256);
    a.encode_traversal(nullptr, 7);

    abnn::Snapshot then = a.snapshot();
    const abnn_snapshot_info info = then.info();
    if (info.captures != 1 || info.n_syn != n_syn || info.scalars.clock != 7 || info.scalars.pass_index != 7 ||
        info.bytes < 11ull * n_syn)
        return fail("Snapshot::info");
    const std::vector<abnn_synapse> rec0 = download(a);
    const std::vector<uint64_t> lf0 = a.last_fired();
    const abnn_scalars sc0 = a.scalars();

    a.encode_traversal(nullptr, 9);
    const std::vector<abnn_synapse> rec1 = download(a);
    const std::vector<uint64_t> lf1 = a.last_fired();
    const abnn_scalars sc1 = a.scalars();

    abnn_diff_config cfgs[2];
    std::memset(cfgs, 0, sizeof(cfgs));
    cfgs[0].lo = -0.05f, cfgs[0].hi = 0.05f, cfgs[0].bins = 64;
    cfgs[1].lo = -1.0f, cfgs[1].hi = 1.0f, cfgs[1].bins = 4096, cfgs[1].dst_first = 256, cfgs[1].dst_count = 256;
    abnn::Snapshot now = a.snapshot();
    uint64_t changed = 0;
    for (int k = 0; k < 2; ++k) {
        const uint64_t words = abnn_snapshot_diff_words(&cfgs[k]);
        if (words != ABNN_DIFF_HEADER_WORDS + cfgs[k].bins) return fail("abnn_snapshot_diff_words", k);
        std::vector<uint64_t> want(words);
        abnn::check(abnn_snapshot_diff_host(&cfgs[k], n_nrn, rec0.data(), rec0.size(), rec1.data(), rec1.size(), want.data()),
                    "abnn_snapshot_diff_host");
        const std::vector<uint64_t> got = a.diff(then, cfgs[k]);
        if (got != want) return fail("Brain::diff != abnn_snapshot_diff_host", k);
        if (a.diff(then, cfgs[k], &now) != want) return fail("the diff of two snapshots", k);
        const abnn::DiffView v(got.data(), cfgs[k]);
        uint64_t bins = 0;
        for (uint32_t i = 0; i < cfgs[k].bins; ++i) bins += v.bins()[i];
        if (v.compared() != n_syn || v.compared() != v.dead_both() + v.killed() + v.revived() + v.rewired() + v.paired() ||
            v.selected() != v.same() + v.changed() || v.changed() != v.up() + v.down() + v.zero() + v.nan() ||
            v.up() + v.down() + v.zero() != v.under() + v.over() + bins || !(v.max_abs() > 0.0f))
            return fail("DiffView", k);
        if (k == 0) changed = v.changed();
    }
    if (changed == 0) return fail("the passes changed no weight");

    a.restore(then);
    if (!same(download(a), rec0) || a.last_fired() != lf0 || !same(a.scalars(), sc0)) return fail("restore");
    a.encode_traversal(nullptr, 9);
    if (!same(download(a), rec1) || a.last_fired() != lf1 || !same(a.scalars(), sc1)) return fail("restore then run");

    abnn_diff_config bad = cfgs[0];
    bad.bins = 0;
    uint64_t out[ABNN_DIFF_HEADER_WORDS + 1];
    if (abnn_snapshot_diff_words(&bad) != 0 ||
        abnn_snapshot_diff(a.handle(), then.handle(), nullptr, &bad, out, 0) != ABNN_ERR_INVALID ||
        abnn_snapshot_restore(a.handle(), then.handle(), 4u) != ABNN_ERR_INVALID)
        return fail("a bad config or a bad `what` was accepted");

    std::printf("{\"ok\": true, \"records\": %llu, \"changed\": %llu, \"bytes\": %llu}\n", (unsigned long long)n_syn,
                (unsigned long long)changed, (unsigned long long)info.bytes);
    return 0;
}
