// Host driver of tests/test_frag_idx_host.py: the shared frag_idx of csrc/q3_frag.h as a host compiler sees it (no HIP
// header, no annotation).  Arguments: K rows; writes frag_idx(m, k, K) for m in [0, rows), k in [0, K) to stdout, row by
// row, as native 64-bit words.
#include "../qwen3_tts_axera_russian_amd/csrc/q3_frag.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const int K = atoi(argv[1]), rows = atoi(argv[2]);
    std::vector<uint64_t> out((size_t)rows * K);
    for (int m = 0; m < rows; m++)
        for (int k = 0; k < K; k++) out[(size_t)m * K + k] = (uint64_t)q3::frag_idx(m, k, K);
    return fwrite(out.data(), 8, out.size(), stdout) == out.size() ? 0 : 1;
}
