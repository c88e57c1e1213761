// census_test.cpp -- TEST PROGRAM: the synapse census through the C++ mirrors
// (abnn::Brain::census, abnn::DeviceBrainEngine::set_census / read_census) on
// config 1 against a host loop over the downloaded records that restates
// abnn.h's definition; the loop's snapshots against Brain::census on a twin
// engine stopped at the same steps.
//   usage: census_test   (tests/test_census_gpu.py; prints one JSON line)
#include <abnn/brain.hpp>
#include <abnn/engine.hpp>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

namespace {

uint32_t order_key(float w)
{
    uint32_t b;
    std::memcpy(&b, &w, 4);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

// abnn.h's census over interchange records, one record at a time
abnn::Census host_census(const std::vector<abnn::SynapsePacked>& syn, const abnn_census_config& c)
{
    abnn::Census r;
    r.records = syn.size();
    r.counts.assign(c.bins, 0);
    r.min = std::numeric_limits<float>::infinity();
    r.max = -std::numeric_limits<float>::infinity();
    const float scale = (float)c.bins / (c.hi - c.lo);
    bool any = false;
    for (const abnn::SynapsePacked& s : syn) {
        if (s.dst == 0xFFFFFFFFu) {
            r.tombstones += 1;
            continue;
        }
        if (c.src_count && !(s.src >= c.src_first && s.src - c.src_first < c.src_count)) continue;
        if (c.dst_count && !(s.dst >= c.dst_first && s.dst - c.dst_first < c.dst_count)) continue;
        r.selected += 1;
        const float w = s.w;
        if (w != w) {
            r.nan += 1;
            continue;
        }
        if (!any || order_key(w) < order_key(r.min)) r.min = w;
        if (!any || order_key(w) > order_key(r.max)) r.max = w;
        any = true;
        if (w < c.lo)
            r.under += 1;
        else if (w >= c.hi)
            r.over += 1;
        else
            r.counts[std::min((uint32_t)((w - c.lo) * scale), c.bins - 1)] += 1;
    }
    return r;
}

bool same(const abnn::Census& a, const abnn::Census& b)
{
    return a.records == b.records && a.tombstones == b.tombstones && a.selected == b.selected && a.under == b.under &&
           a.over == b.over && a.nan == b.nan && std::memcmp(&a.min, &b.min, 4) == 0 &&
           std::memcmp(&a.max, &b.max, 4) == 0 && a.counts == b.counts;
}

std::vector<abnn::SynapsePacked> download(abnn::Brain& b)
{
    std::vector<abnn::SynapsePacked> s(b.n_syn());
    abnn::check(abnn_download_synapses(b.handle(), 0, s.data(), s.size()), "abnn_download_synapses");
    return s;
}

int fail(const char* what, long at = -1)
{
    std::printf("{\"ok\": false, \"what\": \"%s\", \"at\": %ld}\n", what, at);
    return 1;
}

std::shared_ptr<abnn::FunctionalDataset> dataset()
{
    return std::make_shared<abnn::FunctionalDataset>(256, 256, 0.0009, 0.5, abnn::FunctionalDataset::cos_squared,
                                                     abnn::FunctionalDataset::half_sine);
}

}  // namespace

int main()
{
    abnn::Brain a(256, 256, 488, 10000, 100000), b(256, 256, 488, 10000, 100000);  // config 1
    a.build_random_graph(1);
    b.build_random_graph(1);

    // Brain::census against the host loop: no ranges, the dense block, 4096 bins over a narrow span
    const abnn_census_config cfgs[] = {{0.0f, 1.0f, 64, 0, 0, 0, 0, 0},
                                       {0.0f, 1.0f, 64, 0, 256, 256, 256, 0},
                                       {0.15f, 0.5f, 4096, 0, 0, 0, 0, 0},
                                       {0.0f, 1.0f, 7, 300, 100, 0, 0, 0}};
    const std::vector<abnn::SynapsePacked> syn = download(a);
    uint64_t dense = 0;
    for (int k = 0; k < 4; ++k) {
        const abnn::Census got = a.census(cfgs[k]), want = host_census(syn, cfgs[k]);
        if (!same(got, want)) return fail("Brain::census", k);
        if (got.selected != got.under + got.over + got.nan + [&] {
                uint64_t s = 0;
                for (uint64_t x : got.counts) s += x;
                return s;
            }())
            return fail("invariant", k);
        if (k == 1) dense = got.selected;
    }
    if (dense != 10000u) return fail("dense block");  // config 1's 10 000 records all lie in the input->output block

    // the learning loop: a census every 20 steps in a ring of 2, one call of 60 passes
    abnn::EngineConfig ec;
    ec.win_size = 25;
    const abnn_census_config cfg = cfgs[0];
    std::vector<abnn::Census> ring;
    std::vector<uint64_t> steps;
    {
        abnn::DeviceBrainEngine ea(a, ec);
        ea.set_stimulus(dataset());
        ea.set_census(&cfg, 20, 2);
        ea.enqueue_passes(60);
        if (ea.census_count() != 3) return fail("census_count");
        ring = ea.read_census(1, 2, &steps);
        if (steps != std::vector<uint64_t>{40, 60}) return fail("steps");
        bool thrown = false;
        try {
            ea.read_census(0, 1);
        } catch (const std::runtime_error&) {
            thrown = true;
        }
        if (!thrown) return fail("evicted snapshot was readable");
        if (!same(ring[1], host_census(download(a), cfg))) return fail("last snapshot vs the host loop");
    }
    {
        abnn::DeviceBrainEngine eb(b, ec);
        eb.set_stimulus(dataset());
        eb.enqueue_passes(40);
        if (!same(b.census(cfg), ring[0])) return fail("snapshot at step 40");
        eb.enqueue_passes(20);
        if (!same(b.census(cfg), ring[1])) return fail("snapshot at step 60");
    }
    if (a.checksum() != b.checksum()) return fail("the census changed the trajectory");
    if (a.last_fired() != b.last_fired()) return fail("lastFired");

    std::printf("{\"ok\": true, \"records\": %llu, \"dense_selected\": %llu, \"snapshots\": %zu, \"step0\": %llu, "
                "\"step1\": %llu, \"moved\": %s}\n",
                (unsigned long long)ring[1].records, (unsigned long long)dense, ring.size(),
                (unsigned long long)steps[0], (unsigned long long)steps[1],
                same(ring[0], ring[1]) ? "false" : "true");
    return 0;
}
