// matrix_test.cpp -- TEST PROGRAM: the population connectivity matrix through the
// C++ mirrors (abnn::Brain::matrix / matrix_enqueue, abnn::MatrixView) on the
// generated graph against abnn_matrix_host over the downloaded records: the
// built-in populations, 64 equal-width populations with every plane, a weight
// band, and a label plane on the device.
//   usage: matrix_test   (tests/test_matrix_gpu.py; prints one JSON line)
#include <abnn/brain.hpp>

#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>

namespace {

int fail(const char* what, long at = -1)
{
    std::printf("{\"ok\": false, \"what\": \"%s\", \"at\": %ld}\n", what, at);
    return 1;
}

// The HIP runtime is in the process through the library: device memory for the
// label plane without a compile-time dependency on it.
template <class F>
F hip(const char* name)
{
    void* p = dlsym(RTLD_DEFAULT, name);
    if (!p) {
        fail(name);
        std::exit(1);
    }
    return reinterpret_cast<F>(p);
}

}  // namespace

int main()
{
    const uint32_t n_syn = 100000;
    abnn::Brain a(256, 256, 9488, n_syn, 100000);
    a.build_random_graph(1);
    std::vector<abnn_synapse> syn(a.n_syn());
    abnn::check(abnn_download_synapses(a.handle(), 0, syn.data(), syn.size()), "abnn_download_synapses");
    const uint64_t n_nrn = a.n_neuron();
    const uint32_t N = (uint32_t)n_nrn;
    abnn_params params{};
    abnn::check(abnn_get_params(a.handle(), &params), "abnn_get_params");

    const uint32_t io[4] = {0, 256, 512, N};
    uint32_t wide[65];
    for (uint32_t j = 0; j <= 64; ++j) wide[j] = (uint32_t)((uint64_t)N * j / 64);
    const uint32_t inner[3] = {100, 300, N - 7};  // a prefix and a suffix unassigned
    std::vector<uint32_t> labels(n_nrn);
    for (uint32_t n = 0; n < N; ++n) labels[n] = (n % 11 == 0) ? 0xFFFFFFFFu : (n * 2654435761u >> 28) % 9;  // 8 and none: no population

    struct Case {
        abnn_matrix_config cfg;
        const uint32_t* bounds;
    };
    const Case cases[] = {
        {{3, ABNN_MAT_COUNT | ABNN_MAT_W, 0, 0.0f, 0.0f, {0, 0, 0}}, io},
        {{64, ABNN_MAT_COUNT | ABNN_MAT_W | ABNN_MAT_P, 0, 0.0f, 0.0f, {0, 0, 0}}, wide},
        {{2, ABNN_MAT_P, ABNN_MAT_WEIGHT, 0.3f, 0.9f, {0, 0, 0}}, inner},
        {{8, ABNN_MAT_COUNT | ABNN_MAT_P, ABNN_MAT_LABELS, 0.0f, 0.0f, {0, 0, 0}}, nullptr},
    };

    auto hipMalloc = hip<int (*)(void**, size_t)>("hipMalloc");
    auto hipFree = hip<int (*)(void*)>("hipFree");
    auto hipMemcpy = hip<int (*)(void*, const void*, size_t, int)>("hipMemcpy");  // kind 1: to the device, 2: from it
    uint32_t* labels_dev = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&labels_dev), n_nrn * 4) != 0) return fail("hipMalloc");
    if (hipMemcpy(labels_dev, labels.data(), n_nrn * 4, 1) != 0) return fail("hipMemcpy");

    uint64_t hidden_hidden = 0, io_counted = 0, label_counted = 0;
    long k = 0;
    for (const Case& c : cases) {
        const bool lab = c.cfg.flags & ABNN_MAT_LABELS;
        const std::vector<uint64_t> got = a.matrix(c.cfg, c.bounds, lab ? labels_dev : nullptr);
        std::vector<uint64_t> want(abnn_matrix_words(&c.cfg));
        if (got.size() != want.size()) return fail("words", k);
        abnn::check(abnn_matrix_host(syn.data(), syn.size(), &c.cfg, c.bounds, lab ? labels.data() : nullptr, n_nrn,
                                     params.base_scale, want.data(), want.size()),
                    "abnn_matrix_host");
        for (size_t j = 0; j < want.size(); ++j)
            if (got[j] != want[j]) return fail("a word differs from abnn_matrix_host", (long)j);
        const abnn::MatrixView v(got.data(), c.cfg);
        if (v.records() != syn.size() || v.neurons() != n_nrn || v.pops() != c.cfg.pops) return fail("header", k);
        if (v.tombstones() + v.counted() + v.src_unassigned() + v.dst_unassigned() + v.unassigned() + v.out_of_band() != v.records())
            return fail("the classes do not add up", k);
        uint64_t sizes = 0, cells = 0;
        for (uint64_t j = 0; j < v.pops(); ++j) sizes += v.size(j);
        if (sizes != v.assigned()) return fail("sizes", k);
        if (v.plane(ABNN_MAT_COUNT)) {
            for (uint64_t x = 0; x < v.pops(); ++x)
                for (uint64_t y = 0; y < v.pops(); ++y) cells += v.count(x, y);
            if (cells != v.counted()) return fail("the COUNT plane does not sum to word 2", k);
        }
        if ((v.plane(ABNN_MAT_W) != nullptr) != ((c.cfg.what & ABNN_MAT_W) != 0)) return fail("plane view", k);
        if (k == 0) hidden_hidden = v.count(2, 2), io_counted = v.counted();
        if (k == 0 && (v.weight(2, 2) <= 0 || v.counted() != v.records())) return fail("the built-in populations cover every record");
        if (k == 3) label_counted = v.counted();
        k += 1;
    }

    // enqueue only, into device memory, then the same words
    const abnn_matrix_config& c0 = cases[0].cfg;
    const uint64_t words = abnn_matrix_words(&c0);
    uint64_t* out_dev = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&out_dev), words * 8) != 0) return fail("hipMalloc");
    a.matrix_enqueue(c0, io, nullptr, out_dev);
    std::vector<uint64_t> back(words);
    if (hipMemcpy(back.data(), out_dev, words * 8, 2) != 0) return fail("hipMemcpy");  // the null stream follows the kernels
    if (back != a.matrix(c0, io)) return fail("the enqueued matrix");

    bool refused = false;
    try {
        a.matrix(c0, io, labels_dev);  // both partitions
    } catch (const std::runtime_error&) {
        refused = true;
    }
    if (!refused) return fail("two partitions were accepted");
    (void)hipFree(out_dev);
    (void)hipFree(labels_dev);

    std::printf("{\"ok\": true, \"records\": %llu, \"neurons\": %llu, \"hidden_hidden\": %llu, \"io_counted\": %llu, "
                "\"label_counted\": %llu}\n",
                (unsigned long long)syn.size(), (unsigned long long)n_nrn, (unsigned long long)hidden_hidden,
                (unsigned long long)io_counted, (unsigned long long)label_counted);
    return 0;
}
