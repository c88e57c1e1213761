// components_host_test.cpp -- TEST PROGRAM, stand-alone (no HIP, no library):
// the connected components' host rule (abnn_amd/csrc/components.h
// components_host) over the cases of a file, for a build with
// -fsanitize=address,undefined (tests/test_components_abi.py writes the cases
// and compares the results with abnn_amd.components).
//   usage: components_host_test IN OUT
//   IN:  u64 cases; per case { abnn_components_config, u64 n_nrn, n, n abnn_synapse }
//   OUT: per case { abnn_components_words u64 }
#include "../../abnn_amd/csrc/components.h"

#include <cstdio>
#include <vector>

namespace {

bool get(std::FILE* f, void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
bool put(std::FILE* f, const void* p, size_t bytes) { return bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes; }

}  // namespace

int main(int argc, char** argv)
{
    static_assert(sizeof(abnn_components_config) == 32, "abnn.h abnn_components_config");
    if (argc != 3) return 2;
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint64_t cases = 0;
    if (!get(in, &cases, 8)) return 3;
    for (uint64_t k = 0; k < cases; ++k) {
        abnn_components_config cfg;
        uint64_t dims[2];  // n_nrn, n
        if (!get(in, &cfg, sizeof(cfg)) || !get(in, dims, sizeof(dims))) return 3;
        std::vector<abnn_synapse> rec(dims[1]);
        if (!get(in, rec.data(), rec.size() * sizeof(abnn_synapse))) return 3;
        const uint64_t words = abnn::components_words(&cfg, dims[0]);
        if (words == 0) return 4;
        std::vector<uint64_t> res(words);  // exactly the words: a write past them is the sanitizer's
        abnn::components_host(cfg, dims[0], rec.data(), rec.size(), res.data());
        if (!put(out, res.data(), words * 8)) return 5;
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 5;
}
