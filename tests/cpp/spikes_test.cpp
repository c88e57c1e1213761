// spikes_test.cpp -- TEST PROGRAM: the spike recorder (abnn.h abnn_spikes_*)
// through the C++ mirrors (abnn::Brain::record_spikes / spikes_info /
// read_spike_passes / read_spike_raster / read_spike_counts / clear_spikes /
// stop_spikes).
//   1. Against the CPU oracle: one oracle pass run as shard_gate -> shard_apply
//      -> shard_commit at world 1 leaves the pass's spike list in its exchange
//      record; abnn.h's per-pass rule over those lists, restated here, must
//      equal every word the recorder holds (no range with counts, and a range).
//   2. The engine path: the device-resident loop (DeviceBrainEngine) with the
//      recorder on against the host-driven loop BrainEngine<abnn::Brain> with
//      the recorder on, fed the same frames -- the two loops are bit-identical,
//      so pass entries, rasters and counts must be equal -- and against a third
//      run with the recorder off: state, rates and trace unchanged.
//   usage: spikes_test   (tests/test_spikes_gpu.py; prints one JSON line)
#include <abnn/brain.hpp>
#include <abnn/engine.hpp>

#include <cstdio>
#include <cstring>

#include "oracle_brain.hpp"

namespace {

int fail(const char* what, long at = -1)
{
    std::printf("{\"ok\": false, \"what\": \"%s\", \"at\": %ld}\n", what, at);
    return 1;
}

struct Recorded {
    abnn_spikes_info info{};
    std::vector<abnn_spike_pass> passes;
    std::vector<uint32_t> raster, counts;
};

// abnn.h's per-pass rule, one pass at a time
struct HostRule {
    HostRule(const abnn_spikes_config& c, uint64_t n_nrn) : cfg(c)
    {
        if (c.counts) r.counts.assign(c.count ? c.count : n_nrn, 0);
    }
    void pass(const std::vector<uint32_t>& L, uint64_t pass_index, uint64_t now, uint64_t epoch)
    {
        std::vector<uint32_t> S;
        for (uint32_t d : L)
            if (!cfg.count || (d >= cfg.first && d - cfg.first < cfg.count)) S.push_back(d);
        r.info.passes_seen += 1;
        r.info.spikes_seen += L.size();
        r.info.selected_seen += S.size();
        if (cfg.counts)
            for (uint32_t d : S) r.counts[d - (cfg.count ? cfg.first : 0u)] += 1;
        const bool room = cfg.raster_capacity == 0 || r.info.spikes_recorded + S.size() <= cfg.raster_capacity;
        if (!dropped && r.info.passes_recorded < cfg.pass_capacity && room) {
            r.passes.push_back(abnn_spike_pass{pass_index, now, r.info.spikes_recorded, (uint32_t)S.size(), (uint32_t)epoch});
            if (cfg.raster_capacity) r.raster.insert(r.raster.end(), S.begin(), S.end());
            r.info.passes_recorded += 1;
            r.info.spikes_recorded += S.size();
        } else {
            dropped = true;
            r.info.passes_dropped += 1;
            r.info.spikes_dropped += S.size();
        }
    }
    abnn_spikes_config cfg;
    Recorded r;
    bool dropped = false;
};

Recorded read_all(const abnn::Brain& b, const abnn_spikes_config& cfg)
{
    Recorded r;
    r.info = b.spikes_info();
    r.passes = b.read_spike_passes();
    if (cfg.raster_capacity) r.raster = b.read_spike_raster(0, r.info.spikes_recorded);
    if (cfg.counts) r.counts = b.read_spike_counts(cfg.count ? cfg.first : 0u, cfg.count ? cfg.count : b.n_neuron());
    return r;
}

const char* differ(const Recorded& a, const Recorded& b)
{
    if (std::memcmp(&a.info, &b.info, sizeof(a.info)) != 0) return "info";
    if (a.passes.size() != b.passes.size()) return "pass count";
    for (size_t k = 0; k < a.passes.size(); ++k) {
        const abnn_spike_pass &x = a.passes[k], &y = b.passes[k];
        if (x.pass_index != y.pass_index || x.now != y.now || x.offset != y.offset || x.count != y.count ||
            x.epoch != y.epoch)
            return "pass entry";
    }
    if (a.raster != b.raster) return "raster";
    if (a.counts != b.counts) return "counts";
    return nullptr;
}

// One oracle pass through the shard phases at world 1; returns its spike list.
std::vector<uint32_t> oracle_pass_list(OracleBrain& o, std::vector<oracle_g2>& g2, std::vector<int32_t>& xchg)
{
    const int64_t n = oracle_shard_gate(&o.s_, g2.data(), g2.size(), xchg.data());
    if (n < 0) throw std::runtime_error("oracle_shard_gate overflow");
    oracle_shard_apply(&o.s_, g2.data(), n, xchg.data(), 1, 0);
    oracle_shard_commit(&o.s_, xchg.data(), 1);
    int64_t cand = 0;
    std::memcpy(&cand, xchg.data(), 8);
    const uint64_t len = std::min<uint64_t>((uint64_t)cand, o.s_.p.max_spikes);
    const int32_t* sp = xchg.data() + 2 * ABNN_SUMMARY_WORDS;
    return std::vector<uint32_t>(sp, sp + len);
}

std::shared_ptr<abnn::FunctionalDataset> dataset()
{
    return std::make_shared<abnn::FunctionalDataset>(256, 256, 0.0009, 0.5, abnn::FunctionalDataset::cos_squared,
                                                     abnn::FunctionalDataset::half_sine);
}

template <class T>
bool same(const std::vector<T>& a, const std::vector<T>& b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

}  // namespace

int main()
{
    // ---- 1. the mirrors against the oracle's lists ----------------------------------------------
    const uint32_t kPasses = 16;
    const uint64_t n_syn = 100000, events = 100000;
    uint64_t oracle_spikes = 0;
    {
        abnn::Brain all(256, 256, 488, (uint32_t)n_syn, (uint32_t)events), hid(256, 256, 488, (uint32_t)n_syn, (uint32_t)events);
        OracleBrain cpu(256, 256, 488, n_syn, events);
        all.build_random_graph(1);
        hid.build_random_graph(1);
        cpu.build_random_graph(1);
        for (abnn::Brain* b : {&all, &hid}) abnn::check(abnn_set_auto_stimulus(b->handle(), 0, 256), "stimulus");
        cpu.s_.stim_first = 0;
        cpu.s_.stim_count = 256;
        const abnn_spikes_config c_all{1u << 20, 64, 0, 0, 1, {0, 0}}, c_hid{1u << 20, 64, 512, 488, 1, {0, 0}};
        all.record_spikes(c_all);
        hid.record_spikes(c_hid);
        HostRule r_all(c_all, all.n_neuron()), r_hid(c_hid, hid.n_neuron());
        std::vector<oracle_g2> g2(events);
        std::vector<int32_t> xchg(oracle_exchange_words(cpu.s_.p.max_spikes));
        for (uint32_t k = 0; k < kPasses; ++k) {
            const uint64_t pass_index = cpu.s_.pass_index, now = cpu.s_.clock, epoch = cpu.s_.renorms;
            const std::vector<uint32_t> L = oracle_pass_list(cpu, g2, xchg);
            oracle_spikes += L.size();
            r_all.pass(L, pass_index, now, epoch);
            r_hid.pass(L, pass_index, now, epoch);
        }
        all.encode_traversal(nullptr, 5);
        all.encode_traversal(nullptr, kPasses - 5);
        for (uint32_t k = 0; k < kPasses; ++k) hid.encode_traversal();
        if (const char* w = differ(read_all(all, c_all), r_all.r)) return fail(w, 1);
        if (const char* w = differ(read_all(hid, c_hid), r_hid.r)) return fail(w, 2);
        if (all.last_fired() != cpu.all_last_fired()) return fail("lastFired against the oracle");
        if (r_all.r.info.spikes_seen != oracle_spikes || r_hid.r.info.selected_seen == 0 ||
            r_hid.r.info.selected_seen >= oracle_spikes)
            return fail("the shape does not exercise the range");
        // clear re-arms, stop ends it
        all.clear_spikes(true);
        abnn_spikes_info i = all.spikes_info();
        if (i.passes_recorded || i.spikes_recorded || i.passes_seen != kPasses) return fail("clear");
        if (all.read_spike_counts(0, all.n_neuron()) != r_all.r.counts) return fail("clear kept no counts");
        all.stop_spikes();
        bool thrown = false;
        try {
            all.spikes_info();
        } catch (const std::runtime_error&) {
            thrown = true;
        }
        if (!thrown) return fail("a stopped recorder was readable");
    }

    // ---- 2. the engine path ------------------------------------------------------------------------
    const uint32_t kSteps = 300;
    abnn::EngineConfig ec;
    ec.win_size = 50;
    const abnn_spikes_config cfg{(uint64_t)kSteps * 2560, kSteps, 0, 0, 1, {0, 0}};
    abnn::Brain a(256, 256, 488, 10000, 100000), b(256, 256, 488, 10000, 100000), c(256, 256, 488, 10000, 100000);
    for (abnn::Brain* x : {&a, &b, &c}) x->build_random_graph(1);
    a.record_spikes(cfg);
    b.record_spikes(cfg);
    Recorded ra, rb;
    {
        abnn::DeviceBrainEngine ea(a, ec), ecc(c, ec);
        abnn::BrainEngine<abnn::Brain> eb(b, ec);
        ea.set_stimulus(dataset());
        eb.set_stimulus(dataset());
        ecc.set_stimulus(dataset());
        for (uint32_t n : {1u, 7u, 64u, kSteps - 72u}) {  // uneven calls, no synchronise in between
            ea.enqueue_passes(n);
            ecc.enqueue_passes(n);
        }
        for (uint32_t p = 0; p < kSteps; ++p) eb.run_one_pass();
        b.synchronize();
        ra = read_all(a, cfg);
        rb = read_all(b, cfg);
        if (const char* w = differ(ra, rb)) return fail(w, 3);
        if (ra.info.passes_recorded != kSteps || ra.info.passes_dropped != 0) return fail("engine passes recorded");
        if (ra.info.spikes_seen == 0) return fail("the engine run spiked nowhere");
        for (uint32_t p = 0; p < kSteps; ++p)
            if (ra.passes[p].pass_index != p) return fail("engine pass_index", p);
        // the recorder perturbs nothing: the engine with it against the engine without
        std::vector<uint8_t> oa, oc;
        std::vector<float> sa, sc;
        ea.trace(0, kSteps, &oa, &sa);
        ecc.trace(0, kSteps, &oc, &sc);
        if (!same(oa, oc) || !same(sa, sc)) return fail("trace");
        const abnn_engine_state x = ea.state(), y = ecc.state();
        if (x.step != y.step || x.windows != y.windows || x.win_pos != y.win_pos || x.teach != y.teach ||
            std::memcmp(&x.max_observed, &y.max_observed, 4) != 0 || std::memcmp(&x.last_loss, &y.last_loss, 8) != 0 ||
            std::memcmp(&x.last_reward, &y.last_reward, 4) != 0)
            return fail("engine state");
        if (!same(ea.rates(), ecc.rates()) || !same(ea.smooth_rates(), ecc.smooth_rates()) ||
            !same(ea.spike_window(), ecc.spike_window()))
            return fail("rates");
        if (!same(ea.rates(), eb.rates())) return fail("host loop rates");
    }
    if (a.checksum() != c.checksum() || a.checksum() != b.checksum()) return fail("weights");
    if (a.last_fired() != c.last_fired() || a.last_fired() != b.last_fired()) return fail("lastFired");

    std::printf("{\"ok\": true, \"passes\": %u, \"oracle_spikes\": %llu, \"engine_passes\": %llu, \"engine_spikes\": %llu}\n",
                kPasses, (unsigned long long)oracle_spikes, (unsigned long long)ra.info.passes_recorded,
                (unsigned long long)ra.info.spikes_seen);
    return 0;
}
