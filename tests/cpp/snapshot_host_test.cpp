// snapshot_host_test.cpp -- TEST PROGRAM, stand-alone (no HIP, no library): the
// snapshot diff's host rule (abnn_amd/csrc/snapshot.h diff_host) over the cases
// of a file, for a build with -fsanitize=address,undefined
// (tests/test_snapshot_abi.py writes the cases and compares the results with
// abnn_amd.snapshot).
//   usage: snapshot_host_test IN OUT
//   IN:  u64 cases; per case { abnn_diff_config, u64 n_then, n_now,
//        n_then abnn_synapse, n_now abnn_synapse }
//   OUT: per case ABNN_DIFF_HEADER_WORDS + bins u64
#include "../../abnn_amd/csrc/snapshot.h"

#include <cstdio>
#include <vector>

namespace {

bool get(std::FILE* f, void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
bool put(std::FILE* f, const void* p, size_t bytes) { return bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes; }

}  // namespace

int main(int argc, char** argv)
{
    static_assert(sizeof(abnn_diff_config) == 32, "abnn.h abnn_diff_config");
    if (argc != 3) return 2;
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint64_t cases = 0;
    if (!get(in, &cases, 8)) return 3;
    for (uint64_t k = 0; k < cases; ++k) {
        abnn_diff_config cfg;
        uint64_t n[2];  // n_then, n_now
        if (!get(in, &cfg, sizeof(cfg)) || !get(in, n, sizeof(n))) return 3;
        // exact sizes: a read past either side's end is the sanitizer's to find
        std::vector<abnn_synapse> then(n[0]), now(n[1]);
        if (!get(in, then.data(), then.size() * sizeof(abnn_synapse)) ||
            !get(in, now.data(), now.size() * sizeof(abnn_synapse)))
            return 3;
        float scale = 0.0f;
        if (!abnn::diff_config_ok(&cfg, &scale)) return 4;
        std::vector<uint64_t> words(abnn::diff_words(&cfg));
        abnn::diff_host(cfg, scale, then.data(), then.size(), now.data(), now.size(), words.data());
        if (!put(out, words.data(), words.size() * 8)) return 5;
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 5;
}
