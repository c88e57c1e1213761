// matrix_host_test.cpp -- TEST PROGRAM, stand-alone (no HIP, no library): the
// connectivity matrix's host rule (abnn_amd/csrc/matrix.h matrix_host) over the
// cases of a file, for a build with -fsanitize=address,undefined
// (tests/test_matrix_abi.py writes the cases and compares the results with
// abnn_amd.matrix).
//   usage: matrix_host_test IN OUT
//   IN:  u64 cases; per case { abnn_matrix_config, u64 n_nrn, n, f32 base_scale, u32 pad,
//        BOUNDS: P + 1 u32 / LABELS: n_nrn u32, n abnn_synapse }
//   OUT: per case { abnn_matrix_words u64 }
#include "../../abnn_amd/csrc/matrix.h"

#include <cstdio>
#include <vector>

namespace {

bool get(std::FILE* f, void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
bool put(std::FILE* f, const void* p, size_t bytes) { return bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes; }

}  // namespace

int main(int argc, char** argv)
{
    static_assert(sizeof(abnn_matrix_config) == 32, "abnn.h abnn_matrix_config");
    if (argc != 3) return 2;
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint64_t cases = 0;
    if (!get(in, &cases, 8)) return 3;
    for (uint64_t k = 0; k < cases; ++k) {
        abnn_matrix_config cfg;
        uint64_t dims[2];  // n_nrn, n
        float scale[2];    // base_scale, pad
        if (!get(in, &cfg, sizeof(cfg)) || !get(in, dims, sizeof(dims)) || !get(in, scale, sizeof(scale))) return 3;
        const uint64_t words = abnn::matrix_words(&cfg);
        if (words == 0) return 4;
        const bool labels = cfg.flags & ABNN_MAT_LABELS;
        std::vector<uint32_t> part(labels ? dims[0] : cfg.pops + 1);  // exactly the entries the rule may read
        if (!get(in, part.data(), part.size() * 4)) return 3;
        if (!labels && !abnn::matrix_bounds_ok(part.data(), cfg.pops, dims[0])) return 4;
        std::vector<abnn_synapse> rec(dims[1]);
        if (!get(in, rec.data(), rec.size() * sizeof(abnn_synapse))) return 3;
        std::vector<uint64_t> res(words);  // exactly the words: a write past them is the sanitizer's
        abnn::matrix_host(cfg, labels ? nullptr : part.data(), labels ? part.data() : nullptr, dims[0], scale[0], rec.data(),
                          rec.size(), res.data());
        if (!put(out, res.data(), words * 8)) return 5;
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 5;
}
