// learn_bench.cpp -- timing driver of tools/learn_bench.py: learning passes per
// second of (a) the host-driven loop, abnn::BrainEngine<abnn::Brain>::run_one_pass,
// and (b) the device-resident loop, abnn::DeviceBrainEngine in calls of CALL
// passes, alternated REPS times on one brain; after each pair the bare
// traversal (abnn_traverse alone) on the same brain.  Host clock around work
// that ends in a synchronise.
//   usage: learn_bench N_HIDDEN N_SYN EVENTS HOST_PASSES DEVICE_CALLS CALL REPS   (one JSON line)
#include <abnn/brain.hpp>
#include <abnn/engine.hpp>

#include <chrono>
#include <cstdio>
#include <cstdlib>

static std::shared_ptr<abnn::FunctionalDataset> dataset()
{
    return std::make_shared<abnn::FunctionalDataset>(256, 256, 0.0009, 0.5, abnn::FunctionalDataset::cos_squared,
                                                     abnn::FunctionalDataset::half_sine);
}

static double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int main(int argc, char** argv)
{
    if (argc < 8) {
        std::fprintf(stderr, "usage: learn_bench N_HIDDEN N_SYN EVENTS HOST_PASSES DEVICE_CALLS CALL REPS\n");
        return 2;
    }
    const uint32_t n_hid = (uint32_t)std::atoll(argv[1]), n_syn = (uint32_t)std::atoll(argv[2]),
                   events = (uint32_t)std::atoll(argv[3]);
    const uint32_t host_passes = (uint32_t)std::atoi(argv[4]), calls = (uint32_t)std::atoi(argv[5]),
                   call = (uint32_t)std::atoi(argv[6]), reps = (uint32_t)std::atoi(argv[7]);
    if (abnn_device_count() == 0) {
        std::fprintf(stderr, "learn_bench needs a HIP device\n");
        return 1;
    }
    abnn::Brain brain(256, 256, n_hid, n_syn, events);
    brain.build_random_graph(1);
    abnn::EngineConfig cfg;  // the reference's defaults (win_size 1000)
    abnn::BrainEngine<abnn::Brain> host(brain, cfg);
    abnn::DeviceBrainEngine dev(brain, cfg, call);
    host.set_stimulus(dataset());
    dev.set_stimulus(dataset());

    // warm-up: each loop and the bare pass once (first launches, the partition settling)
    for (uint32_t k = 0; k < 64; ++k) host.run_one_pass();
    dev.enqueue_passes(call);
    brain.encode_traversal(nullptr, 64);
    brain.synchronize();

    std::printf("{\"n_hidden\": %u, \"n_syn\": %u, \"events\": %u, \"host_passes\": %u, \"device_passes\": %u, "
                "\"call\": %u, \"reps\": [",
                n_hid, n_syn, events, host_passes, calls * call, call);
    for (uint32_t r = 0; r < reps; ++r) {
        double t0 = now_s();
        for (uint32_t k = 0; k < host_passes; ++k) host.run_one_pass();  // every pass ends synchronised
        const double ta = (now_s() - t0) / host_passes;
        t0 = now_s();
        for (uint32_t k = 0; k < calls; ++k) dev.enqueue_passes(call);
        brain.synchronize();
        const double tb = (now_s() - t0) / ((double)calls * call);
        t0 = now_s();
        brain.encode_traversal(nullptr, calls * call);
        brain.synchronize();
        const double tc = (now_s() - t0) / ((double)calls * call);
        std::printf("%s{\"host_us\": %.3f, \"device_us\": %.3f, \"bare_us\": %.3f}", r ? ", " : "", ta * 1e6, tb * 1e6,
                    tc * 1e6);
    }
    const abnn_engine_state s = dev.state();
    std::printf("], \"device_steps\": %llu, \"host_steps\": %llu}\n", (unsigned long long)s.step,
                (unsigned long long)host.step());
    return 0;
}
