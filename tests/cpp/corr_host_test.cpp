// corr_host_test -- the correlograms' host rule (csrc/corr.h alone: no HIP, no
// library) in a stand-alone program, built with -fsanitize=address,undefined
// (abnn_amd/build.py build_corr_host_test).  A few hundred random cases: empty
// rows, K == 0, a window that starts past K, a table whose last row is clamped
// to the raster.  Every case runs the three modes and checks the identities
// between them: the PAIRS matrix summed over its cells is POP, SYNAPSES is the
// sum of M_all[src][dst] over the followed records, word 4 is the plane's sum.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../abnn_amd/csrc/corr.h"

using namespace abnn;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n)  // [0, n)
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return n ? (uint32_t)(g_state >> 33) % n : 0;
}

static int fail(int c, const char* what)
{
    std::fprintf(stderr, "case %d: %s\n", c, what);
    return 1;
}

int main()
{
    int cases = 0;
    for (int c = 0; c < 300; ++c) {
        const uint32_t n_nrn = 1 + rnd(24);
        const uint32_t K = c % 17 == 0 ? 0 : 1 + rnd(10);
        std::vector<abnn_spike_pass> passes(K);
        std::vector<uint32_t> raster;
        for (uint32_t k = 0; k < K; ++k) {
            const uint32_t n = rnd(3) == 0 ? 0 : rnd(7);  // empty rows
            passes[k] = abnn_spike_pass{k, k, raster.size(), n, 0};
            for (uint32_t i = 0; i < n; ++i) raster.push_back(rnd(4) == 0 ? rnd(2) : rnd(n_nrn));
        }
        uint64_t cap = raster.size();
        if (K && c % 5 == 0) {  // the last row claims more than the raster holds: clamped
            passes[K - 1].count += 3 + rnd(5);
            if (c % 10 == 0) passes[K - 1].offset = cap + 7;  // or starts past it: empty
        }
        std::vector<abnn_synapse> rec(rnd(60));
        for (auto& r : rec) {
            r = abnn_synapse{};
            r.src = rnd(n_nrn);
            r.dst = rnd(n_nrn);
            r.w = (float)rnd(100) / 100.0f;
            if (rnd(8) == 0) r.src = r.dst = 0xFFFFFFFFu;
            if (rnd(16) == 0) r.src = n_nrn + rnd(3);  // never validated: not followed
        }
        abnn_corr_config cfg{};
        cfg.max_lag = c % 3 == 0 ? 0 : rnd(13);
        if (rnd(2)) {
            cfg.a_first = rnd(n_nrn);
            cfg.a_count = 1 + rnd(n_nrn - cfg.a_first);
        }
        if (rnd(2)) {
            cfg.b_first = rnd(n_nrn);
            cfg.b_count = 1 + rnd(n_nrn - cfg.b_first);
        }
        if (rnd(3) == 0) {
            cfg.row_first = c % 7 == 0 ? K + rnd(3) : rnd(K + 1);  // also past K
            cfg.row_count = rnd(K + 2);
        }
        if (rnd(3) == 0) {
            cfg.flags = ABNN_CORR_WEIGHT;
            cfg.w_lo = 0.25f;
            cfg.w_hi = 0.75f;
        }
        const uint32_t flags = cfg.flags;
        const float w_lo = cfg.w_lo, w_hi = cfg.w_hi;
        const uint64_t nb = 2ull * cfg.max_lag + 1;

        cfg.mode = ABNN_CORR_SYNAPSES;
        if (corr_words(&cfg) != 8 + nb || !corr_ranges_ok(cfg, n_nrn)) return fail(c, "synapses config");
        std::vector<uint64_t> syn(8 + nb);
        corr_host(cfg, n_nrn, passes.data(), K, raster.data(), cap, rec.data(), rec.size(), syn.data());

        cfg.mode = ABNN_CORR_POP;
        cfg.flags = 0;
        cfg.w_lo = cfg.w_hi = 0.0f;
        std::vector<uint64_t> pop(8 + nb);
        corr_host(cfg, n_nrn, passes.data(), K, raster.data(), cap, nullptr, 0, pop.data());

        // every pair of neurons: A and B as the whole brain
        abnn_corr_config all = cfg;
        all.mode = ABNN_CORR_PAIRS;
        all.a_first = all.b_first = 0;
        all.a_count = all.b_count = n_nrn;
        if (corr_words(&all) != 8 + (uint64_t)n_nrn * n_nrn * nb) return fail(c, "pairs config");
        std::vector<uint64_t> m(8 + (uint64_t)n_nrn * n_nrn * nb);
        corr_host(all, n_nrn, passes.data(), K, raster.data(), cap, nullptr, 0, m.data());

        const CorrRule rule = [&] {
            abnn_corr_config s = cfg;
            s.mode = ABNN_CORR_SYNAPSES;
            s.flags = flags;
            s.w_lo = w_lo;
            s.w_hi = w_hi;
            return corr_rule(s, n_nrn);
        }();
        std::vector<uint64_t> want_pop(nb), want_syn(nb);
        uint64_t followed = 0, coupled = 0;
        for (uint32_t x = 0; x < n_nrn; ++x)
            for (uint32_t y = 0; y < n_nrn; ++y)
                if (corr_in_a(rule, x) && corr_in_b(rule, y))
                    for (uint64_t l = 0; l < nb; ++l) want_pop[l] += m[8 + ((uint64_t)x * n_nrn + y) * nb + l];
        for (const auto& r : rec) {
            uint32_t wbits;
            __builtin_memcpy(&wbits, &r.w, 4);
            if (!corr_followed(rule, r.src, r.dst, wbits)) continue;
            ++followed;
            uint64_t add = 0;
            for (uint64_t l = 0; l < nb; ++l) {
                const uint64_t v = m[8 + ((uint64_t)r.src * n_nrn + r.dst) * nb + l];
                want_syn[l] += v;
                add += v;
            }
            coupled += add ? 1 : 0;
        }
        uint64_t sum_pop = 0, sum_syn = 0, sum_m = 0;
        for (uint64_t l = 0; l < nb; ++l) {
            if (pop[8 + l] != want_pop[l]) return fail(c, "POP != the PAIRS matrix summed over its cells");
            if (syn[8 + l] != want_syn[l]) return fail(c, "SYNAPSES != the sum of M_all[src][dst]");
            sum_pop += pop[8 + l];
            sum_syn += syn[8 + l];
        }
        for (size_t i = 8; i < m.size(); ++i) sum_m += m[i];
        if (pop[4] != sum_pop || syn[4] != sum_syn || m[4] != sum_m) return fail(c, "word 4 != the plane's sum");
        if (syn[5] != followed || syn[6] != coupled || pop[5] || pop[6]) return fail(c, "followed / coupled");
        for (int w : {0, 1, 2, 3, 7})
            if (pop[w] != syn[w]) return fail(c, "the header's window words differ between the modes");
        if (pop[7] != K || pop[0] > K || m[1] != pop[1]) return fail(c, "rows / K");
        if (cfg.row_first >= K && (pop[0] || pop[1] || sum_pop)) return fail(c, "a window past K is empty");
        ++cases;
    }
    std::printf("corr_host_test: %d cases ok\n", cases);
    return 0;
}
