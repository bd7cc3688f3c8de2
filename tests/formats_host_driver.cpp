// formats_host_driver.cpp -- the native weight-file readers (csrc/q3_formats.cpp, Pack::open_bytes in csrc/q3_common.cpp)
// behind a job list, for tests/test_native_formats_malformed.py.  Built with -fsanitize=address,undefined and run on the
// CPU: it calls no HIP function and opens no device (the HIP runtime is linked only because q3_common.cpp's device-selection
// entry points name it).
//
//   formats_host_driver jobs <file>      one job per line of <file>:
//       npy|npz|safetensors|container <path> [heap | trunc N]
//           the file (heap: all of it, the default; trunc N: its first N bytes) is copied into a malloc'd buffer of exactly
//           that size -- so the sanitizer sees the first byte read past its end, which it cannot for a mapping -- and parsed
//           through the bytes-level entry into a fresh Pack (.npy under the name "t", .npz / .safetensors through the
//           reference-key maps)
//       auto <path> [aux_dir]
//           Pack::open_auto(path, aux_dir): the directory logic and the trimming of the codec tables
//     -> per job "job <line>" (flushed before the parse, so that a crash names its input), then "refused", or
//        "accepted <n tensors>", the inventory lines q3t_inspect_weights prints ("name dtype ndim d0 d1 d2 d3 fnv1a64", "meta
//        key value") and "end".  Before it prints `accepted` it checks every tensor in 128-bit arithmetic -- ndim <= 4, a
//        known dtype, nbytes == numel * element size, [data, data + nbytes) inside the input buffer, one of Pack::owned or
//        (auto) one of the Pack's mappings -- and exits with status 3 and a message if one fails; the hash reads every byte.
//   formats_host_driver fp16             h2f on all 65536 patterns and f2h_sat on four sets of floats against the compiler's
//                                        _Float16 conversions; one line per set, status 1 on a mismatch
#include "../qwen3_tts_axera_russian_amd/csrc/q3_common.h"

#include <cmath>
#include <fstream>
#include <sstream>

using namespace q3;

typedef unsigned __int128 u128;

static bool inside(const uint8_t* d, uint64_t nb, const uint8_t* base, size_t size) {
    if (!base) return false;
    const uintptr_t a = (uintptr_t)d, b = (uintptr_t)base;
    return a >= b && (u128)(a - b) + nb <= (u128)size;
}

// -> "" or what is wrong with the tensor
static std::string inconsistent(const Pack& pk, const PackTensor& t, const uint8_t* buf, size_t n) {
    static const uint64_t esz[5] = {4, 2, 4, 8, 2};
    if (t.ndim > 4) return "ndim > 4";
    if (t.dtype > 4) return "unknown dtype";
    bool zero = false;
    for (uint32_t i = 0; i < t.ndim; i++) zero |= t.shape[i] == 0;
    u128 ne = zero ? 0 : 1;
    for (uint32_t i = 0; i < t.ndim && !zero; i++) {
        ne *= t.shape[i];                            // < 2^64 * 2^64
        if (ne >> 64) return "numel does not fit 64 bits";
    }
    if ((u128)t.nbytes != ne * esz[t.dtype]) return "nbytes != numel * element size";
    if (t.nbytes == 0) return "";
    if (!t.data) return "null data";
    if (inside(t.data, t.nbytes, buf, n) || inside(t.data, t.nbytes, pk.map, pk.map_size)) return "";
    for (const auto& o : pk.owned)
        if (inside(t.data, t.nbytes, o.data(), o.size())) return "";
    for (const auto& m : pk.extra_maps)
        if (inside(t.data, t.nbytes, m.first, m.second)) return "";
    return "data outside the input and every owned buffer";
}

// a name as one word: bytes that would split a line or a field are written \xNN (no name of a sound file has one)
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
        printf("%s %u %u %llu %llu %llu %llu %llx\n", word(t.name).c_str(), t.dtype, t.ndim, (unsigned long long)t.shape[0],
               (unsigned long long)t.shape[1], (unsigned long long)t.shape[2], (unsigned long long)t.shape[3], h);
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
            bool ok;
            if (fmt == "npy") ok = pk.add_npy_bytes(buf, n, "t", path.c_str());
            else if (fmt == "npz") ok = pk.add_npz_bytes(buf, n, path.c_str(), map_cp_npz_key);
            else if (fmt == "safetensors") ok = pk.add_safetensors_bytes(buf, n, path.c_str(), map_safetensors_key);
            else if (fmt == "container") ok = pk.open_bytes(buf, n, path.c_str());
            else {
                fprintf(stderr, "unknown format in job: %s\n", line.c_str());
                free(buf);
                return 2;
            }
            if (!ok) printf("refused\n");
            else rc = report(pk, buf, n);
        }
        free(buf);
        if (rc) return rc;
    }
    return 0;
}

// ---- h2f / f2h_sat against the compiler's _Float16 ----
static uint16_t bits16(_Float16 h) {
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}
static _Float16 half_of(uint16_t u) {
    _Float16 h;
    memcpy(&h, &u, 2);
    return h;
}
static uint32_t bits32(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
static float float_of(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

static long long g_bad = 0;

// f2h_sat(f) against (_Float16)clamp(f, +-65504); NaN -> 0x7e00
static void check_f2h(float f) {
    uint16_t want;
    if (f != f) {
        want = 0x7e00;
    } else {
        volatile float c = f > 65504.f ? 65504.f : f < -65504.f ? -65504.f : f;
        want = bits16((_Float16)c);
    }
    const uint16_t got = f2h_sat(f);
    if (got != want && g_bad++ < 10) fprintf(stderr, "f2h_sat(%a = 0x%08x) = 0x%04x, the compiler's is 0x%04x\n", f, bits32(f), got, want);
}
static void check_f2h_with_neighbours(float f) {
    check_f2h(f);
    check_f2h(nextafterf(f, -INFINITY));
    check_f2h(nextafterf(f, INFINITY));
}

static int run_fp16() {
    long long n = 0;
    for (uint32_t u = 0; u < 65536; u++, n++) {
        volatile _Float16 h = half_of((uint16_t)u);
        const float want = (float)h, got = h2f((uint16_t)u);
        const bool same = want != want ? got != got : bits32(want) == bits32(got);
        if (!same && g_bad++ < 10) fprintf(stderr, "h2f(0x%04x) = 0x%08x, the compiler's is 0x%08x\n", u, bits32(got), bits32(want));
    }
    printf("h2f patterns %lld\n", n);
    n = 0;
    for (uint32_t u = 0; u < 65536; u++) {           // every half value as a float, with its two float neighbours
        if ((u & 0x7c00) == 0x7c00) continue;        // (inf and NaN: the edge set)
        volatile _Float16 h = half_of((uint16_t)u);
        check_f2h_with_neighbours((float)h);
        n += 3;
    }
    printf("f2h_sat halves %lld\n", n);
    n = 0;
    for (uint32_t u = 0; u < 65536; u++) {           // every midpoint between adjacent halves (a tie), with its two neighbours
        if ((u & 0x7fff) >= 0x7bff) continue;        // (above 65504 there is no finite neighbour: 65520 is in the edge set)
        volatile _Float16 a = half_of((uint16_t)u), b = half_of((uint16_t)(u + 1));
        const float mid = 0.5f * ((float)a + (float)b);   // 12 significant bits: exact
        check_f2h_with_neighbours(mid);
        n += 3;
    }
    printf("f2h_sat midpoints %lld\n", n);
    n = 0;
    for (uint32_t u = 0; u < 65536; u++, n++) check_f2h(float_of(u << 16));   // every bf16 value
    printf("f2h_sat bf16 %lld\n", n);
    n = 0;
    const float edges[] = {INFINITY, -INFINITY, NAN, -NAN, float_of(0x7f800001u), float_of(0xffc12345u), 65504.f, -65504.f,
                           65519.99f, -65519.99f, 65520.f, -65520.f, 65536.f, 3.4e38f, -3.4e38f, 0.f, -0.f};
    for (float f : edges) {
        check_f2h_with_neighbours(f);
        n += 3;
    }
    // what the contract names outright, whatever the compiler does there
    if (f2h_sat(INFINITY) != 0x7bff || f2h_sat(-INFINITY) != 0xfbff || f2h_sat(NAN) != 0x7e00 || f2h_sat(65520.f) != 0x7bff ||
        f2h_sat(65519.99f) != 0x7bff || f2h_sat(65504.f) != 0x7bff) {
        fprintf(stderr, "f2h_sat: the saturation edge is off\n");
        g_bad++;
    }
    printf("f2h_sat edges %lld\n", n);
    printf("mismatches %lld\n", g_bad);
    return g_bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && std::string(argv[1]) == "jobs") return run_jobs(argv[2]);
    if (argc == 2 && std::string(argv[1]) == "fp16") return run_fp16();
    fprintf(stderr, "usage: %s jobs <file> | fp16\n", argv[0]);
    return 2;
}
