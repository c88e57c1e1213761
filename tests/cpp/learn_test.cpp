// learn_test.cpp -- TEST PROGRAM: the device-resident learning loop
// (abnn::DeviceBrainEngine over abnn.h's abnn_engine_*) on the GPU brain against
// the host driver BrainEngine<OracleBrain> on the CPU oracle, bit for bit:
// every pass's output spikes and normalised rates (the trace), last_loss and
// last_reward at every call boundary, and at the end all weights, all of
// lastFired, clock / rBar / reward, rate, smooth, spike_window, max_observed,
// step, windows.  The GPU side runs the passes in uneven chunks with no
// synchronise between the calls (handle A); the call-boundary values need a
// synchronise, so they are read on a second handle (B) run with the same chunks.
//   usage: learn_test CASE   (1..8, tests/test_learn_gpu.py; prints one JSON line)
#include <abnn/brain.hpp>
#include <abnn/engine.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "oracle_brain.hpp"

namespace {

// The oracle adapter, counting what the driver writes through it.
struct CountingOracle : OracleBrain {
    using OracleBrain::OracleBrain;
    void set_timestamps(const std::vector<uint32_t>& idx, uint64_t v)
    {
        teacher_stamps += idx.size();
        OracleBrain::set_timestamps(idx, v);
    }
    void set_reward(float r)
    {
        if (std::memcmp(&r, &s_.reward, 4) != 0) ++reward_changes;
        OracleBrain::set_reward(r);
    }
    uint64_t teacher_stamps = 0, reward_changes = 0;
};

struct Case {
    uint32_t n_in, n_out;
    uint64_t n_hid, n_syn, events;
    uint32_t passes;
    abnn::EngineConfig cfg;
    uint64_t renorm_thresh;  // 0: the default
    bool hand_back;
    void (*knobs)(abnn_params&) = nullptr;  // brain knobs off the defaults
    uint64_t cap_extra = 0;                 // syn_capacity = n_syn + cap_extra (structural plasticity)
};

Case make_case(int id)
{
    Case c{256, 256, 488, 10000, 100000, 300, {}, 0, false};  // config 1
    c.cfg.win_size = 50;
    switch (id) {
        case 1: break;
        case 2:  // odd sizes, renormalisation mid-run, a FIR ring and a window that divide nothing
            c = Case{70, 300, 630, 30000, 30000, 130, {}, 40, false};
            c.cfg.win_size = 40;
            c.cfg.fir_size = 7;
            break;
        case 3:
            c.passes = 90;
            c.cfg.win_size = 30;
            c.cfg.use_fir = false;
            break;
        case 4:  // more than one gate workgroup
            c = Case{256, 256, 99488, 2000000, 2000000, 60, {}, 0, false};
            c.cfg.win_size = 25;
            break;
        case 5:  // hand-back to the host paths after 40 engine passes
            c.passes = 40;
            c.hand_back = true;
            break;
        case 6:  // off the default knobs: a clock that skips, the widest incremental window, weights above 1
            // (with clock_inc = 2 read_outputs' window [now - 1, now) can hold no stamp: the loop
            // and the host driver must agree on that as on everything else)
            c.passes = 120;
            c.cfg.win_size = 30;
            c.renorm_thresh = 50;
            c.knobs = [](abnn_params& p) {
                p.clock_inc = 2;
                p.window_pre = 7;
                p.tick_ns = 500;
                p.w_max = 2.0f;
            };
            break;
        case 7:  // no earlier spike list in the window, a reward term that moves the weights
            c.passes = 120;
            c.cfg.win_size = 30;
            c.renorm_thresh = 50;
            c.knobs = [](abnn_params& p) {
                p.clock_inc = 1;
                p.window_pre = 1;
                p.tick_ns = 500;
                p.w_max = 2.0f;
                p.eta_reward = 0.5f;
            };
            break;
        case 8:  // structural plasticity: an update after every 7th pass, so in the middle of the 7-, 64- and
            // 48-pass calls (the synchronising host part of the update inside abnn_engine_run)
            c.passes = 120;
            c.cfg.win_size = 30;
            c.cap_extra = 2000;
            c.knobs = [](abnn_params& p) {
                p.w_prune = 0.105f;
                p.p_new = 0.35f;
                p.w_init = 0.5f;
                p.compact_every = 7;
            };
            break;
        default: std::fprintf(stderr, "unknown case %d\n", id); std::exit(2);
    }
    return c;
}

std::shared_ptr<abnn::FunctionalDataset> dataset(const Case& c)
{
    // the app's stimulus (view-delegate.cpp:32-42): cos^2 input, 0.5 sin + 0.5 target
    return std::make_shared<abnn::FunctionalDataset>(c.n_in, c.n_out, 0.0009, 0.5,
                                                     abnn::FunctionalDataset::cos_squared,
                                                     abnn::FunctionalDataset::half_sine);
}

std::vector<uint32_t> chunks_of(uint32_t passes)
{
    std::vector<uint32_t> ch;
    for (uint32_t c : {1u, 7u, 64u}) {
        if (passes == 0) break;
        const uint32_t n = std::min(c, passes);
        ch.push_back(n);
        passes -= n;
    }
    if (passes) ch.push_back(passes);
    return ch;
}

template <class T>
bool same(const std::vector<T>& a, const std::vector<T>& b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

int fail(const char* what, long at = -1)
{
    std::printf("{\"ok\": false, \"what\": \"%s\", \"at\": %ld}\n", what, at);
    return 1;
}

bool brain_matches(abnn::Brain& gpu, CountingOracle& cpu, const char** what)
{
    const std::vector<abnn_synapse> ref = cpu.synapses();  // the first n_syn records
    const uint64_t n_syn = ref.size();
    if (gpu.n_syn() != n_syn) return *what = "n_syn", false;
    std::vector<abnn::SynapsePacked> w(n_syn);
    abnn::check(abnn_download_synapses(gpu.handle(), 0, reinterpret_cast<abnn_synapse*>(w.data()), n_syn), "download");
    if (n_syn && std::memcmp(w.data(), ref.data(), n_syn * sizeof(abnn_synapse)) != 0) return *what = "synapses", false;
    if (gpu.last_fired() != cpu.all_last_fired()) return *what = "last_fired", false;
    const abnn_scalars sg = gpu.scalars(), sc = cpu.scalars();
    if (sg.clock != sc.clock) return *what = "clock", false;
    if (std::memcmp(&sg.rbar, &sc.rbar, 4) != 0) return *what = "rbar", false;
    if (std::memcmp(&sg.reward, &sc.reward, 4) != 0) return *what = "reward", false;
    return true;
}

}  // namespace

int main(int argc, char** argv)
{
    const int id = argc > 1 ? std::atoi(argv[1]) : 1;
    const Case c = make_case(id);
    abnn_params params;
    abnn_default_params(&params);
    if (c.renorm_thresh) params.renorm_thresh = c.renorm_thresh;
    if (c.knobs) c.knobs(params);

    abnn::Brain gpu_a(c.n_in, c.n_out, (uint32_t)c.n_hid, (uint32_t)c.n_syn, (uint32_t)c.events, 0, &params,
                      c.n_syn + c.cap_extra);
    abnn::Brain gpu_b(c.n_in, c.n_out, (uint32_t)c.n_hid, (uint32_t)c.n_syn, (uint32_t)c.events, 0, &params,
                      c.n_syn + c.cap_extra);
    CountingOracle cpu(c.n_in, c.n_out, c.n_hid, c.n_syn, c.events, &params, c.n_syn + c.cap_extra);
    gpu_a.build_random_graph(1);
    gpu_b.build_random_graph(1);
    cpu.build_random_graph(1);

    // the reference driver on the oracle, recorded pass by pass
    abnn::BrainEngine<CountingOracle> ec(cpu, c.cfg);
    ec.set_stimulus(dataset(c));
    const uint32_t no = c.n_out;
    std::vector<uint8_t> ref_out((size_t)c.passes * no);
    std::vector<float> ref_smooth((size_t)c.passes * no);
    std::vector<double> ref_loss(c.passes);
    std::vector<float> ref_reward(c.passes);
    uint64_t spikes = 0;
    for (uint32_t p = 0; p < c.passes; ++p) {
        const std::vector<bool> o = ec.run_one_pass();
        for (uint32_t i = 0; i < no; ++i) spikes += (ref_out[(size_t)p * no + i] = o[i] ? 1 : 0);
        std::memcpy(&ref_smooth[(size_t)p * no], ec.smooth_rates().data(), no * sizeof(float));
        ref_loss[p] = ec.last_loss();
        ref_reward[p] = ec.last_reward();
    }

    const std::vector<uint32_t> chunks = chunks_of(c.passes);
    {
        // handle A: every call enqueued with no synchronise in between
        abnn::DeviceBrainEngine ea(gpu_a, c.cfg);
        ea.set_stimulus(dataset(c));
        for (uint32_t n : chunks) ea.enqueue_passes(n);
        std::vector<uint8_t> out;
        std::vector<float> smooth;
        ea.trace(0, c.passes, &out, &smooth);
        for (uint32_t p = 0; p < c.passes; ++p) {
            if (std::memcmp(&out[(size_t)p * no], &ref_out[(size_t)p * no], no) != 0) return fail("outputs", p);
            if (std::memcmp(&smooth[(size_t)p * no], &ref_smooth[(size_t)p * no], no * 4) != 0) return fail("rates", p);
        }
        const abnn_engine_state s = ea.state();
        const float mo = ec.max_observed(), lr = ec.last_reward();
        const double ll = ec.last_loss();
        if (s.step != ec.step() || s.step != c.passes) return fail("step");
        if (s.windows != ec.windows()) return fail("windows");
        if (std::memcmp(&s.max_observed, &mo, 4) != 0) return fail("max_observed");
        if (std::memcmp(&s.last_reward, &lr, 4) != 0) return fail("last_reward");
        if (std::memcmp(&s.last_loss, &ll, 8) != 0) return fail("last_loss");
        if (s.teach != (c.passes & 1u)) return fail("teach");
        if (s.win_pos != c.passes % c.cfg.win_size) return fail("win_pos");
        if (!same(ea.rates(), ec.rates())) return fail("rate");
        if (!same(ea.smooth_rates(), ec.smooth_rates())) return fail("smooth");
        if (!same(ea.spike_window(), ec.spike_window())) return fail("spike_window");
        const char* what = "";
        if (!brain_matches(gpu_a, cpu, &what)) return fail(what);

        // handle B: the same calls, loss and reward read at every call boundary
        abnn::DeviceBrainEngine eb(gpu_b, c.cfg);
        eb.set_stimulus(dataset(c));
        uint32_t done = 0;
        for (uint32_t n : chunks) {
            eb.enqueue_passes(n);
            done += n;
            const abnn_engine_state sb = eb.state();
            if (std::memcmp(&sb.last_loss, &ref_loss[done - 1], 8) != 0) return fail("boundary loss", done);
            if (std::memcmp(&sb.last_reward, &ref_reward[done - 1], 4) != 0) return fail("boundary reward", done);
        }
        if (gpu_b.checksum() != gpu_a.checksum()) return fail("handle B's weights");
        if (gpu_b.last_fired() != gpu_a.last_fired()) return fail("handle B's lastFired");
    }

    bool inject_ok = true, resume_ok = true;
    if (c.hand_back) {
        // one host inject_inputs on both sides: the handle's RNG went on where the all-host driver's would be
        const std::vector<float> frame = dataset(c)->nextInput();
        gpu_a.inject_inputs(frame, 1000.0f);
        cpu.inject_inputs(frame, 1000.0f);
        inject_ok = gpu_a.last_fired(0, c.n_in) == cpu.last_fired(0, c.n_in);
        if (!inject_ok) return fail("inject after the run");
        // plain passes with no host write: the incremental bitmap build resumes
        for (int k = 0; k < 8; ++k) {
            gpu_a.encode_traversal();
            cpu.encode_traversal();
        }
        gpu_a.synchronize();
        const char* what = "";
        resume_ok = brain_matches(gpu_a, cpu, &what);
        if (!resume_ok) return fail(what, 8);
    }

    abnn_stats st{};
    abnn::check(abnn_get_stats(gpu_a.handle(), &st), "abnn_get_stats");
    if (!c.hand_back && (st.pruned != cpu.s_.stats.pruned || st.grown != cpu.s_.stats.grown)) return fail("pruned / grown");
    std::printf("{\"ok\": true, \"case\": %d, \"passes\": %u, \"spikes\": %llu, \"teacher_stamps\": %llu, "
                "\"windows\": %llu, \"reward_changes\": %llu, \"renorms_gpu\": %llu, \"renorms_cpu\": %llu, "
                "\"structural_updates\": %llu, \"pruned\": %llu, \"grown\": %llu, \"n_syn\": %llu, "
                "\"loss\": %.17g, \"reward\": %.9g}\n",
                id, c.passes, (unsigned long long)spikes, (unsigned long long)cpu.teacher_stamps,
                (unsigned long long)ec.windows(), (unsigned long long)cpu.reward_changes,
                (unsigned long long)abnn_renormalisations(gpu_a.handle()), (unsigned long long)cpu.s_.renorms,
                (unsigned long long)abnn_structural_updates(gpu_a.handle()), (unsigned long long)st.pruned,
                (unsigned long long)st.grown, (unsigned long long)gpu_a.n_syn(), ec.last_loss(), ec.last_reward());
    return 0;
}
