// edit_host_test.cpp -- TEST PROGRAM, stand-alone (no HIP, no library): the
// synapse edit's host rule (abnn_amd/csrc/edit.h edit_host / edit_factors_host)
// over the cases of a file, for a build with -fsanitize=address,undefined
// (tests/test_edit_abi.py writes the cases and compares the results with
// abnn_amd.edit).
//   usage: edit_host_test IN OUT
//   IN:  u64 cases; per case { abnn_edit_config, u64 n_nrn, syn_offset, n, m,
//        n abnn_synapse, m f32 (the plane; m = 0: none) }; then u64 count,
//        f32 target, f_lo, f_hi, pad, count u64 strength words
//   OUT: per case { 8 u64 header, n abnn_synapse }; then count f32 factors
#include "../../abnn_amd/csrc/edit.h"

#include <cstdio>
#include <cstring>
#include <vector>

namespace {

bool get(std::FILE* f, void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
bool put(std::FILE* f, const void* p, size_t bytes) { return bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes; }

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint64_t cases = 0;
    if (!get(in, &cases, 8)) return 3;
    for (uint64_t k = 0; k < cases; ++k) {
        abnn_edit_config cfg;
        uint64_t dims[4];  // n_nrn, syn_offset, n, m
        if (!get(in, &cfg, sizeof(cfg)) || !get(in, dims, sizeof(dims))) return 3;
        std::vector<abnn_synapse> rec(dims[2]);
        std::vector<float> plane(dims[3]);
        if (!get(in, rec.data(), rec.size() * sizeof(abnn_synapse)) || !get(in, plane.data(), plane.size() * 4)) return 3;
        if (!abnn::edit_config_ok(&cfg) || abnn::edit_plane_count(cfg, dims[0]) != dims[3]) return 4;
        uint64_t head[ABNN_EDIT_HEADER_WORDS];
        abnn::edit_host(cfg, dims[0], dims[1], rec.data(), rec.size(), plane.empty() ? nullptr : plane.data(), head);
        if (!put(out, head, sizeof(head)) || !put(out, rec.data(), rec.size() * sizeof(abnn_synapse))) return 5;
    }
    uint64_t count = 0;
    float par[4];
    if (!get(in, &count, 8) || !get(in, par, sizeof(par))) return 3;
    std::vector<uint64_t> words(count);
    std::vector<float> factors(count);
    if (!get(in, words.data(), count * 8)) return 3;
    if (!abnn::edit_factors_ok(par[0], par[1], par[2])) return 4;
    abnn::edit_factors_host(words.data(), count, par[0], par[1], par[2], factors.data());
    if (!put(out, factors.data(), count * 4)) return 5;
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 5;
}
