// reorder_host_test.cpp -- TEST PROGRAM, stand-alone (no HIP, no library): the
// record reorder's host rule (abnn_amd/csrc/reorder.h reorder_host) over the
// cases of a file, for a build with -fsanitize=address,undefined
// (tests/test_reorder_abi.py writes the cases and compares the results with
// abnn_amd.reorder).
//   usage: reorder_host_test IN OUT
//   IN:  u64 cases; per case { abnn_reorder_config, u64 syn_offset, n, m,
//        n abnn_synapse, m u32 (the perm; m = 0: none; m = n with PERM) }
//   OUT: per case { abnn_reorder_words u64, n abnn_synapse }
#include "../../abnn_amd/csrc/reorder.h"

#include <cstdio>
#include <cstring>
#include <vector>

namespace {

bool get(std::FILE* f, void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
bool put(std::FILE* f, const void* p, size_t bytes) { return bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes; }

}  // namespace

int main(int argc, char** argv)
{
    static_assert(sizeof(abnn_reorder_config) == 32, "abnn.h abnn_reorder_config");
    if (argc != 3) return 2;
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint64_t cases = 0;
    if (!get(in, &cases, 8)) return 3;
    for (uint64_t k = 0; k < cases; ++k) {
        abnn_reorder_config cfg;
        uint64_t dims[3];  // syn_offset, n, m
        if (!get(in, &cfg, sizeof(cfg)) || !get(in, dims, sizeof(dims))) return 3;
        std::vector<abnn_synapse> rec(dims[1]);
        std::vector<uint32_t> perm(dims[2] + 1);  // never empty: PERM over no record still has a pointer
        if (!get(in, rec.data(), rec.size() * sizeof(abnn_synapse)) || !get(in, perm.data(), dims[2] * 4)) return 3;
        const bool has_perm = cfg.key == ABNN_REORDER_PERM;
        const uint64_t words = abnn::reorder_words(&cfg, dims[1]);
        if (words == 0 || (has_perm && dims[2] != dims[1]) || (!has_perm && dims[2] != 0)) return 4;
        std::vector<uint64_t> res(words);
        abnn::reorder_host(cfg, dims[0], rec.data(), rec.size(), has_perm ? perm.data() : nullptr, res.data());
        if (!put(out, res.data(), words * 8) || !put(out, rec.data(), rec.size() * sizeof(abnn_synapse))) return 5;
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 5;
}
