// gguf_host_driver.cpp -- the native GGUF reader (Pack::add_gguf_bytes, Pack::open_auto in csrc/q3_formats.cpp) behind a job
// list, for tests/test_gguf_format.py.  Built with -fsanitize=address,undefined and run on the CPU as a program of its own:
// it calls no HIP function and opens no device (the HIP runtime is linked only because q3_common.cpp's device-selection
// entry points name it).
//
//   gguf_host_driver jobs <file>      one job per line of <file>:
//       gguf <path> [heap | trunc N]
//           the file (heap: all of it, the default; trunc N: its first N bytes) is copied into a malloc'd buffer of exactly
//           that size -- so the sanitizer sees the first byte read past its end -- and parsed by add_gguf_bytes through
//           map_gguf_key into a fresh Pack
//       auto <path> [aux_dir]
//           Pack::open_auto(path, aux_dir): a .gguf file, a directory, the .npy tables of aux_dir
//     -> per job "job <line>" (flushed before the parse, so that a crash names its input), then "refused", or
//        "accepted <n tensors>", one line per tensor "name dtype ndim d0 d1 d2 d3 offset nbytes fnv1a64" (offset: of the
//        data in the input, -1 when it lies in another buffer), "meta key value" lines and "end".  Before it prints
//        `accepted` it checks every tensor in 128-bit arithmetic -- ndim <= 4, a known dtype, the row length a multiple of
//        the block, nbytes == numel / block elements * block bytes, [data, data + nbytes) inside the input buffer, one of
//        Pack::owned or one of the Pack's mappings -- and exits with status 3 and a message if one fails; the hash reads
//        every byte.
#include "../qwen3_tts_axera_russian_amd/csrc/q3_common.h"

#include <fstream>
#include <sstream>

using namespace q3;

typedef unsigned __int128 u128;

static bool inside(const uint8_t* d, uint64_t nb, const uint8_t* base, size_t size) {
    if (!base) return false;
    const uintptr_t a = (uintptr_t)d, b = (uintptr_t)base;
    return a >= b && (u128)(a - b) + nb <= (u128)size;
}

static std::string inconsistent(const Pack& pk, const PackTensor& t, const uint8_t* buf, size_t n) {
    if (t.ndim > 4) return "ndim > 4";
    const BlockGeom g = block_geom(t.dtype);
    if (!g.elems) return "unknown dtype";
    bool zero = false;
    for (uint32_t i = 0; i < t.ndim; i++) zero |= t.shape[i] == 0;
    u128 ne = zero ? 0 : 1;
    for (uint32_t i = 0; i < t.ndim && !zero; i++) {
        ne *= t.shape[i];
        if (ne >> 64) return "numel does not fit 64 bits";
    }
    if (t.ndim && t.shape[t.ndim - 1] % g.elems) return "row length is no multiple of the block";
    if ((u128)t.nbytes != ne / g.elems * g.bytes) return "nbytes != numel / block elements * block bytes";
    if (is_block_dtype(t.dtype) && t.ndim != 2) return "a block type that is not a matrix";
    if (t.nbytes == 0) return "";
    if (!t.data) return "null data";
    if (inside(t.data, t.nbytes, buf, n) || inside(t.data, t.nbytes, pk.map, pk.map_size)) return "";
    for (const auto& o : pk.owned)
        if (inside(t.data, t.nbytes, o.data(), o.size())) return "";
    for (const auto& m : pk.extra_maps)
        if (inside(t.data, t.nbytes, m.first, m.second)) return "";
    return "data outside the input and every owned buffer";
}

static std::string word(const std::string& s) {
    std::string w;
    char x[8];
    for (unsigned char c : s) {
        if (c > 0x20 && c < 0x7f) {
            w.push_back((char)c);
        } else {
            snprintf(x, sizeof(x), "\\x%02x", c);
            w += x;
        }
    }
    return w.empty() ? "\\x" : w;
}

static int report(const Pack& pk, const uint8_t* buf, size_t n) {
    for (const auto& kv : pk.tensors) {
        const std::string bad = inconsistent(pk, kv.second, buf, n);
        if (!bad.empty()) {
            fflush(stdout);
            fprintf(stderr, "inconsistent tensor %s: %s (dtype %u ndim %u shape %llu %llu %llu %llu nbytes %llu)\n", kv.first.c_str(),
                    bad.c_str(), kv.second.dtype, kv.second.ndim, (unsigned long long)kv.second.shape[0],
                    (unsigned long long)kv.second.shape[1], (unsigned long long)kv.second.shape[2],
                    (unsigned long long)kv.second.shape[3], (unsigned long long)kv.second.nbytes);
            return 3;
        }
    }
    printf("accepted %zu\n", pk.tensors.size());
    for (const auto& kv : pk.tensors) {
        const PackTensor& t = kv.second;
        unsigned long long h = 1469598103934665603ull;
        for (uint64_t i = 0; i < t.nbytes; i++) h = (h ^ t.data[i]) * 1099511628211ull;
        const long long off = buf && inside(t.data, t.nbytes, buf, n) ? (long long)(t.data - buf) : -1;
        printf("%s %u %u %llu %llu %llu %llu %lld %llu %llx\n", word(t.name).c_str(), t.dtype, t.ndim, (unsigned long long)t.shape[0],
               (unsigned long long)t.shape[1], (unsigned long long)t.shape[2], (unsigned long long)t.shape[3], off,
               (unsigned long long)t.nbytes, h);
    }
    for (const auto& kv : pk.meta) printf("meta %s %.17g\n", word(kv.first).c_str(), kv.second);
    printf("end\n");
    return 0;
}

static int run_jobs(const char* list) {
    std::ifstream in(list);
    if (!in) {
        fprintf(stderr, "cannot read the job list %s\n", list);
        return 2;
    }
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string fmt, path, opt;
        if (!(ls >> fmt >> path)) continue;
        printf("job %s\n", line.c_str());
        fflush(stdout);
        if (fmt == "auto") {
            std::string aux;
            ls >> aux;
            Pack pk;
            if (!pk.open_auto(path.c_str(), aux.empty() ? nullptr : aux.c_str())) {
                printf("refused\n");
                continue;
            }
            if (int rc = report(pk, nullptr, 0)) return rc;
            continue;
        }
        if (fmt != "gguf") {
            fprintf(stderr, "unknown format in job: %s\n", line.c_str());
            return 2;
        }
        std::ifstream f(path, std::ios::binary);
        if (!f) {
            fprintf(stderr, "cannot read %s\n", path.c_str());
            return 2;
        }
        std::string bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        size_t n = bytes.size();
        if (ls >> opt && opt == "trunc") {
            unsigned long long k = 0;
            if (!(ls >> k) || k > n) {
                fprintf(stderr, "bad trunc in job: %s\n", line.c_str());
                return 2;
            }
            n = (size_t)k;
        } else if (!opt.empty() && opt != "heap") {
            fprintf(stderr, "unknown option in job: %s\n", line.c_str());
            return 2;
        }
        uint8_t* buf = (uint8_t*)malloc(n);   // exactly n bytes: of a 0-byte input nothing may be read
        if (n) memcpy(buf, bytes.data(), n);
        int rc = 0;
        {
            Pack pk;
            if (!pk.add_gguf_bytes(buf, n, path.c_str(), map_gguf_key)) printf("refused\n");
            else rc = report(pk, buf, n);
        }
        free(buf);
        if (rc) return rc;
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && std::string(argv[1]) == "jobs") return run_jobs(argv[2]);
    fprintf(stderr, "usage: %s jobs <file>\n", argv[0]);
    return 2;
}
