// q3_common.h -- shared host-side helpers for the MI355X Qwen3-TTS libraries.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#define Q3_LOG(...)                              \
    do {                                         \
        fprintf(stderr, "[qwen3tts] " __VA_ARGS__); \
        fputc('\n', stderr);                     \
    } while (0)

// HIP call that makes the enclosing function return `ret` on failure.
#define Q3_HIP(call, ret)                                                              \
    do {                                                                               \
        hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess) {                                                        \
            Q3_LOG("%s:%d: %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
            return ret;                                                                \
        }                                                                              \
    } while (0)

namespace q3 {

typedef _Float16 half_t;

// ---------------------------------------------------------------------------
// Q3TTSW1 container (written by weights.py)
// ---------------------------------------------------------------------------
enum DType : uint32_t {
    F32 = 0, F16 = 1, I32 = 2, I64 = 3,
    BF16 = 4,                                           // safetensors and GGUF only (q3_formats.cpp)
    Q4_0 = 5, Q8_0 = 6, Q4_K = 7, Q5_K = 8, Q6_K = 9    // ggml block types, GGUF only: raw blocks, dequantised on the GPU at load
};
// Elements and bytes of one block of a dtype (1 element for the plain types); {0, 0} for an unknown dtype.
struct BlockGeom {
    uint32_t elems, bytes;
};
inline BlockGeom block_geom(uint32_t dtype) {
    static const BlockGeom g[10] = {{1, 4}, {1, 2}, {1, 4}, {1, 8}, {1, 2}, {32, 18}, {32, 34}, {256, 144}, {256, 176}, {256, 210}};
    return dtype < 10 ? g[dtype] : BlockGeom{0, 0};
}
inline bool is_block_dtype(uint32_t dtype) { return dtype >= Q4_0 && dtype <= Q6_K; }

struct PackTensor {
    std::string name;
    uint32_t dtype = 0, ndim = 0;
    uint64_t shape[4] = {0, 0, 0, 0};
    uint64_t offset = 0, nbytes = 0;
    const uint8_t* data = nullptr;  // into the mapping
    uint64_t numel() const {
        uint64_t n = 1;
        for (uint32_t i = 0; i < ndim; i++) n *= shape[i];
        return n;
    }
    // bytes of one row (the innermost dimension) of a validated tensor; a block type's K is a multiple of its block
    uint64_t row_bytes() const {
        const BlockGeom g = block_geom(dtype);
        return ndim && g.elems ? shape[ndim - 1] / g.elems * g.bytes : 0;
    }
    // The same for a shape that has not been validated yet (a file's): false when the product does not fit 64 bits.
    bool numel_checked(uint64_t* out) const {
        uint64_t n = 1;
        for (uint32_t i = 0; i < ndim; i++)
            if (shape[i] == 0) {
                *out = 0;
                return true;
            }
        for (uint32_t i = 0; i < ndim; i++)
            if (__builtin_mul_overflow(n, shape[i], &n)) return false;
        *out = n;
        return true;
    }
};

struct Pack {
    std::map<std::string, double> meta;
    std::map<std::string, PackTensor> tensors;
    uint8_t* map = nullptr;
    size_t map_size = 0;
    int fd = -1;

    bool open(const char* path);
    // the reference's deployed files instead of a container (q3_formats.cpp): .npy / .npz / .safetensors / .gguf
    // parsed natively, names mapped to the container's; `aux_dir` = the servers' --embeddings_dir
    bool open_auto(const char* path, const char* aux_dir = nullptr);
    bool add_npy(const char* path, const std::string& name);
    bool add_npz(const char* path, std::string (*rename)(const std::string&));
    bool add_safetensors(const char* path, std::string (*rename)(const std::string&));
    bool add_gguf(const char* path, std::string (*rename)(const std::string&));   // the talker's GGUF (v2 / v3, little-endian)
    // The parsers proper: everything above maps its file and calls one of these on the mapping.  They read nothing outside
    // [p, p + n), refuse (false, with a Q3_LOG line) what does not fit there, and let no exception out.  Tensors point into
    // [p, p + n) or into `owned`, so the bytes must outlive the Pack's use.
    bool add_npy_bytes(const uint8_t* p, size_t n, const std::string& name, const char* what);
    bool add_npz_bytes(const uint8_t* p, size_t n, const char* what, std::string (*rename)(const std::string&));
    bool add_safetensors_bytes(const uint8_t* p, size_t n, const char* what, std::string (*rename)(const std::string&));
    bool add_gguf_bytes(const uint8_t* p, size_t n, const char* what, std::string (*rename)(const std::string&));
    bool open_bytes(const uint8_t* p, size_t n, const char* what);   // a Q3TTSW1 container
    const uint8_t* map_file(const char* path, size_t* size);
    std::vector<std::pair<uint8_t*, size_t>> extra_maps;   // files mapped by the add_* readers
    std::vector<std::vector<uint8_t>> owned;                // inflated / converted arrays
    void close();
    ~Pack() { close(); }
    const PackTensor* find(const std::string& n) const {
        auto it = tensors.find(n);
        return it == tensors.end() ? nullptr : &it->second;
    }
    double get(const char* key, double dflt) const {
        auto it = meta.find(key);
        return it == meta.end() ? dflt : it->second;
    }
};

std::string map_cp_npz_key(const std::string& k);
std::string map_safetensors_key(const std::string& k);
std::string map_gguf_key(const std::string& k);   // llama.cpp's qwen3 tensor names

inline float bf16_to_f32(uint16_t b) {
    uint32_t u = (uint32_t)b << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// host fp16 <-> fp32 (round to nearest even, saturating to +-65504)
float h2f(uint16_t h);
uint16_t f2h_sat(float f);

// ---------------------------------------------------------------------------
// What the carry-state objects (VocIncr, EncStream), the encoder handle and the engine share
// ---------------------------------------------------------------------------
// Owner of device allocations: it frees what it handed out, and `bytes` is the sum of the sizes asked for.
struct DeviceAllocs {
    std::vector<void*> ptrs;
    size_t bytes = 0;
    DeviceAllocs() = default;
    DeviceAllocs(const DeviceAllocs&) = delete;
    DeviceAllocs& operator=(const DeviceAllocs&) = delete;
    ~DeviceAllocs() { release(); }
    // *p = n bytes -> false on failure (what it got stays owned)
    template <class T>
    bool alloc(T** p, size_t n) {
        if (hipMalloc((void**)p, n) != hipSuccess) return false;
        ptrs.push_back(*p);
        bytes += n;
        return true;
    }
    // the same, zeroed on stream s: the stream is named at every call, and the caller waits for it before the first use
    template <class T>
    bool alloc_zeroed(T** p, size_t n, hipStream_t s) { return alloc(p, n) && hipMemsetAsync(*p, 0, n, s) == hipSuccess; }
    void adopt(DeviceAllocs& o) {   // everything o owns becomes this one's
        ptrs.insert(ptrs.end(), o.ptrs.begin(), o.ptrs.end());
        bytes += o.bytes;
        o.ptrs.clear();
        o.bytes = 0;
    }
    void release() {
        for (void* p : ptrs) hipFree(p);
        ptrs.clear();
        bytes = 0;
    }
};

// The same for pinned host memory (the engine's read-back staging): it frees what it handed out.
struct PinnedAllocs {
    std::vector<void*> ptrs;
    PinnedAllocs() = default;
    PinnedAllocs(const PinnedAllocs&) = delete;
    PinnedAllocs& operator=(const PinnedAllocs&) = delete;
    ~PinnedAllocs() {
        for (void* p : ptrs) hipHostFree(p);
    }
    template <class T>
    bool alloc(T** p, size_t n) {
        if (hipHostMalloc((void**)p, n, 0) != hipSuccess) return false;
        ptrs.push_back(*p);
        return true;
    }
};

// The entries of a push that run as one launch sequence: those with equal keys, at most max_members to a group.
struct PushGroups {
    std::vector<std::vector<long long>> keys;   // per group
    std::vector<std::vector<int>> members;      // per group: entry indices
    void add(const std::vector<long long>& key, int entry, int max_members) {   // the first group with this key and room, else a new one
        size_t g = 0;
        while (g < keys.size() && (keys[g] != key || (int)members[g].size() >= max_members)) g++;
        if (g == keys.size()) {
            keys.push_back(key);
            members.emplace_back();
        }
        members[g].push_back(entry);
    }
};

struct ModelCfg {
    int hidden = 1024, head_dim = 128, n_heads = 16, n_kv = 8;
    int talker_layers = 28, talker_ffn = 3072, talker_vocab = 3072;
    int cp_layers = 5, cp_ffn = 3072, cp_vocab = 2048, cp_groups = 15;
    float eps = 1e-6f;
    double rope_theta = 1e6;
    int codec_eos = 2150;
    void from_pack(const Pack& p);
};

}  // namespace q3
