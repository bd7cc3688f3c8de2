// q3_formats.cpp -- native readers for the on-disk formats the reference deploys, so the libraries
// start from the reference's own files without Python:
//   .npy  v1/v2/v3, little-endian f4 / f8 (converted) / f2 / i4 / i8, C order
//         (the reference's C++ server parses f4/f8 v1/v2: dual_npu/code_predictor_cpp/npy_reader.h:22-108)
//   .npz  zip of .npy members, stored (np.savez: scripts/export_code_predictor_weights.py:76) or deflated
//         (np.savez_compressed: scripts/extract_embeddings.py:93), zip64 extras tolerated
//   .safetensors  8-byte header length + JSON table + raw tensors (F32 / F16 / BF16), zero-copy from the mapping
//   .gguf  v2 / v3 little-endian: the talker file the reference's server is started with (llamacpp_talker_server.py:379);
//         F32 / F16 / BF16 and the raw blocks of Q4_0 / Q8_0 / Q4_K / Q5_K / Q6_K, zero-copy (dequantised on the GPU at load)
// and the key maps from the reference's names to the container names (weights.py):
//   code_predictor_weights.npz   layer_{i}_{part}, final_norm, codec_emb_{g}, lm_head_{g}
//                                (scripts/export_code_predictor_weights.py:51-74)
//   model.safetensors            HF keys talker.model.layers.*, talker.code_predictor.* (scripts/extract_embeddings.py:47-98)
//                                or the re-keyed Qwen3 talker model.layers.* (scripts/extract_talker_as_qwen3.py:53-71)
//   embeddings/*.npy             codec_embedding.npy, codec_head.npy (scripts/extract_embeddings.py:62-72)
//   *.gguf                       llama.cpp's qwen3 names blk.{i}.attn_q.weight, token_embd.weight, ... (map_gguf_key)
#include "q3_common.h"

#include <exception>

#include <dirent.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

namespace q3 {

namespace {

bool ends_with(const std::string& s, const char* suf) {
    const size_t n = strlen(suf);
    return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

// ---- .npy header -----------------------------------------------------------------------------
// Fills dtype / shape of `t` and returns the offset of the data, or 0 on error.  f8 is reported as
// dtype 100 (the caller converts).
size_t npy_header(const uint8_t* p, size_t n, PackTensor& t, std::string& err) {
    if (n < 10 || memcmp(p, "\x93NUMPY", 6) != 0) {
        err = "not an .npy file (bad magic)";
        return 0;
    }
    const int major = p[6];
    size_t hlen, hoff;
    if (major == 1) {
        hlen = (size_t)p[8] | ((size_t)p[9] << 8);
        hoff = 10;
    } else if (major == 2 || major == 3) {
        if (n < 12) {
            err = "truncated .npy header";
            return 0;
        }
        hlen = (size_t)p[8] | ((size_t)p[9] << 8) | ((size_t)p[10] << 16) | ((size_t)p[11] << 24);
        hoff = 12;
    } else {
        err = "unsupported .npy version " + std::to_string(major);
        return 0;
    }
    if (hoff + hlen > n) {
        err = "truncated .npy header";
        return 0;
    }
    const std::string h((const char*)p + hoff, hlen);
    auto value_after = [&](const char* key) -> size_t {
        size_t k = h.find(std::string("'") + key + "'");
        if (k == std::string::npos) k = h.find(std::string("\"") + key + "\"");
        if (k == std::string::npos) return std::string::npos;
        k = h.find(':', k);
        return k == std::string::npos ? k : k + 1;
    };
    size_t d = value_after("descr");
    if (d == std::string::npos) {
        err = ".npy header lacks descr";
        return 0;
    }
    size_t q0 = h.find_first_of("'\"", d);
    size_t q1 = q0 == std::string::npos ? q0 : h.find_first_of("'\"", q0 + 1);
    if (q1 == std::string::npos) {
        err = ".npy header: structured dtypes are not supported";
        return 0;
    }
    const std::string descr = h.substr(q0 + 1, q1 - q0 - 1);
    if (descr == "<f4" || descr == "=f4") t.dtype = F32;
    else if (descr == "<f2" || descr == "=f2") t.dtype = F16;
    else if (descr == "<i4" || descr == "=i4") t.dtype = I32;
    else if (descr == "<i8" || descr == "=i8") t.dtype = I64;
    else if (descr == "<f8" || descr == "=f8") t.dtype = 100;
    else {
        err = ".npy dtype " + descr + " is not supported (f4, f8, f2, i4, i8 little-endian are)";
        return 0;
    }
    size_t f = value_after("fortran_order");
    if (f != std::string::npos) {   // the key may be absent; its value may not
        f = h.find_first_not_of(' ', f);   // npos when the header ends after the colon
        if (f != std::string::npos && h.compare(f, 4, "True") == 0) {
            err = ".npy fortran_order=True is not supported";
            return 0;
        }
        if (f == std::string::npos || h.compare(f, 5, "False") != 0) {
            err = ".npy header: fortran_order has no value";
            return 0;
        }
    }
    size_t s = value_after("shape");
    size_t lp = s == std::string::npos ? s : h.find('(', s);
    size_t rp = lp == std::string::npos ? lp : h.find(')', lp);
    if (rp == std::string::npos) {
        err = ".npy header lacks shape";
        return 0;
    }
    t.ndim = 0;
    for (size_t i = lp + 1; i < rp;) {
        while (i < rp && (h[i] == ' ' || h[i] == ',')) i++;
        if (i >= rp) break;
        uint64_t v = 0;
        bool any = false;
        while (i < rp && h[i] >= '0' && h[i] <= '9') {
            if (__builtin_mul_overflow(v, (uint64_t)10, &v) || __builtin_add_overflow(v, (uint64_t)(h[i] - '0'), &v)) {
                err = ".npy shape: a dimension does not fit 64 bits";
                return 0;
            }
            i++;
            any = true;
        }
        if (!any || t.ndim >= 4) {
            err = ".npy shape: more than 4 dimensions or malformed";
            return 0;
        }
        t.shape[t.ndim++] = v;
    }
    return hoff + hlen;
}

// ---- minimal JSON (safetensors header) --------------------------------------------------------
struct JTensor {
    std::string dtype;
    std::vector<uint64_t> shape;
    uint64_t begin = 0, end = 0;
};
struct JParser {
    const char* p;
    const char* e;
    bool ok = true;
    void ws() {
        while (p < e && (*p == ' ' || *p == '\n' || *p == '\t' || *p == '\r')) p++;
    }
    bool eat(char c) {
        ws();
        if (p < e && *p == c) {
            p++;
            return true;
        }
        return false;
    }
    std::string str() {
        ws();
        std::string s;
        if (p >= e || *p != '"') {
            ok = false;
            return s;
        }
        p++;
        while (p < e && *p != '"') {
            if (*p == '\\' && p + 1 < e) p++;   // names here carry no escapes worth decoding
            s.push_back(*p++);
        }
        if (p >= e) ok = false;
        else p++;
        return s;
    }
    uint64_t num() {
        ws();
        uint64_t v = 0;
        bool any = false;
        while (p < e && *p >= '0' && *p <= '9') {
            if (__builtin_mul_overflow(v, (uint64_t)10, &v) || __builtin_add_overflow(v, (uint64_t)(*p - '0'), &v)) {
                ok = false;   // a shape or an offset that does not fit 64 bits
                return 0;
            }
            p++;
            any = true;
        }
        if (!any) ok = false;
        return v;
    }
    // Any JSON value (used for __metadata__ and unknown keys of a tensor).  It recurses per nesting level, so the depth is
    // limited: the format's __metadata__ is a flat string -> string map (depth 1) and a tensor's entry has depth 2, while
    // a header of nothing but '[' would otherwise use one stack frame per byte.  Every turn of the loop consumes input.
    static constexpr int kMaxDepth = 32;
    void skip_value(int depth = 0) {
        ws();
        if (p >= e || depth > kMaxDepth) {
            ok = false;
            return;
        }
        if (*p == '"') {
            str();
        } else if (*p == '{' || *p == '[') {
            const char open = *p, close = open == '{' ? '}' : ']';
            p++;
            if (eat(close)) return;
            while (ok) {
                if (open == '{') {
                    str();
                    if (!eat(':')) ok = false;
                }
                if (ok) skip_value(depth + 1);
                if (!ok || eat(close)) return;
                if (!eat(',')) ok = false;
            }
        } else {   // a number, true, false, null: at least one character
            const char* s = p;
            while (p < e && *p != ',' && *p != '}' && *p != ']' && *p != ' ' && *p != '\n' && *p != '\t' && *p != '\r') p++;
            if (p == s) ok = false;
        }
    }
    bool tensor(JTensor& t) {
        if (!eat('{')) return false;
        while (ok && !eat('}')) {
            const std::string k = str();
            if (!eat(':')) return false;
            if (k == "dtype") {
                t.dtype = str();
            } else if (k == "shape") {
                if (!eat('[')) return false;
                while (ok && !eat(']')) {
                    t.shape.push_back(num());
                    eat(',');
                }
            } else if (k == "data_offsets") {
                if (!eat('[')) return false;
                t.begin = num();
                if (!eat(',')) return false;
                t.end = num();
                if (!eat(']')) return false;
            } else {
                skip_value();
            }
            eat(',');
        }
        return ok;
    }
};

// ---- name maps ---------------------------------------------------------------------------------
const char* const kLayerParts[] = {"input_ln", "q_proj", "k_proj", "v_proj", "o_proj", "q_norm",
                                   "k_norm",   "post_ln", "gate_proj", "up_proj", "down_proj"};
const char* const kHfParts[] = {"input_layernorm.weight",     "self_attn.q_proj.weight", "self_attn.k_proj.weight",
                                "self_attn.v_proj.weight",    "self_attn.o_proj.weight", "self_attn.q_norm.weight",
                                "self_attn.k_norm.weight",    "post_attention_layernorm.weight",
                                "mlp.gate_proj.weight",       "mlp.up_proj.weight",      "mlp.down_proj.weight"};

bool split_int(const std::string& s, size_t pos, int& v, size_t& next) {
    v = 0;
    size_t i = pos;
    while (i < s.size() && s[i] >= '0' && s[i] <= '9') v = v * 10 + (s[i++] - '0');
    next = i;
    return i > pos;
}

// "<prefix>{i}.<hf part>" -> "<stack>.layers.{i}.<part>"
std::string map_hf_layer(const std::string& k, const char* prefix, const char* stack) {
    const size_t n = strlen(prefix);
    if (k.compare(0, n, prefix) != 0) return "";
    int i;
    size_t nx;
    if (!split_int(k, n, i, nx) || nx >= k.size() || k[nx] != '.') return "";
    const std::string rest = k.substr(nx + 1);
    for (int p = 0; p < 11; p++)
        if (rest == kHfParts[p]) return std::string(stack) + ".layers." + std::to_string(i) + "." + kLayerParts[p];
    return "";
}

}  // namespace

// code_predictor_weights.npz member (without ".npy") -> container name
std::string map_cp_npz_key(const std::string& k) {
    int i;
    size_t nx;
    if (k.compare(0, 6, "layer_") == 0 && split_int(k, 6, i, nx) && nx < k.size() && k[nx] == '_') {
        const std::string part = k.substr(nx + 1);
        for (const char* p : kLayerParts)
            if (part == p) return "cp.layers." + std::to_string(i) + "." + part;
        return "";
    }
    if (k == "final_norm") return "cp.norm";
    if (k.compare(0, 10, "codec_emb_") == 0 && split_int(k, 10, i, nx) && nx == k.size()) return "cp.codec_emb." + std::to_string(i);
    if (k.compare(0, 8, "lm_head_") == 0 && split_int(k, 8, i, nx) && nx == k.size()) return "cp.lm_head." + std::to_string(i);
    return "";
}

// safetensors key (HF checkpoint, or the re-keyed Qwen3 talker) -> container name
std::string map_safetensors_key(const std::string& k) {
    std::string r = map_hf_layer(k, "talker.model.layers.", "talker");
    if (!r.empty()) return r;
    r = map_hf_layer(k, "model.layers.", "talker");
    if (!r.empty()) return r;
    r = map_hf_layer(k, "talker.code_predictor.model.layers.", "cp");
    if (!r.empty()) return r;
    if (k == "talker.model.norm.weight" || k == "model.norm.weight") return "talker.norm";
    if (k == "talker.model.codec_embedding.weight" || k == "model.embed_tokens.weight") return "talker.codec_embedding";
    if (k == "talker.codec_head.weight" || k == "lm_head.weight") return "talker.codec_head";
    if (k == "talker.code_predictor.model.norm.weight") return "cp.norm";
    int i;
    size_t nx;
    const char* e = "talker.code_predictor.model.codec_embedding.";
    if (k.compare(0, strlen(e), e) == 0 && split_int(k, strlen(e), i, nx) && k.substr(nx) == ".weight")
        return "cp.codec_emb." + std::to_string(i);
    const char* h = "talker.code_predictor.lm_head.";
    if (k.compare(0, strlen(h), h) == 0 && split_int(k, strlen(h), i, nx) && k.substr(nx) == ".weight")
        return "cp.lm_head." + std::to_string(i);
    if (k == "talker.model.text_embedding.weight") return "text.embedding";
    if (k == "talker.text_projection.linear_fc1.weight") return "text.fc1.weight";
    if (k == "talker.text_projection.linear_fc1.bias") return "text.fc1.bias";
    if (k == "talker.text_projection.linear_fc2.weight") return "text.fc2.weight";
    if (k == "talker.text_projection.linear_fc2.bias") return "text.fc2.bias";
    return "";
}

const uint8_t* Pack::map_file(const char* path, size_t* size) {
    int f = ::open(path, O_RDONLY);
    if (f < 0) return nullptr;
    struct stat st;
    if (fstat(f, &st) != 0 || st.st_size <= 0) {
        ::close(f);
        return nullptr;
    }
    void* m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, f, 0);
    ::close(f);
    if (m == MAP_FAILED) return nullptr;
    extra_maps.push_back({(uint8_t*)m, (size_t)st.st_size});
    *size = (size_t)st.st_size;
    return (const uint8_t*)m;
}

bool Pack::add_npy_bytes(const uint8_t* p, size_t n, const std::string& name, const char* what) try {
    PackTensor t;
    std::string err;
    const size_t off = npy_header(p, n, t, err);   // <= n
    if (!off) {
        Q3_LOG("%s: %s", what, err.c_str());
        return false;
    }
    t.name = name;
    uint64_t ne;
    if (!t.numel_checked(&ne)) {
        Q3_LOG("%s: the shape's element count does not fit 64 bits", what);
        return false;
    }
    if (t.dtype == 100) {   // f8 -> f4, as the reference's reader does
        if (ne > (n - off) / 8) {
            Q3_LOG("%s: truncated data", what);
            return false;
        }
        owned.emplace_back((size_t)ne * 4);
        float* dst = (float*)owned.back().data();
        for (uint64_t i = 0; i < ne; i++) {
            double v;
            memcpy(&v, p + off + i * 8, 8);
            dst[i] = (float)v;
        }
        t.dtype = F32;
        t.data = owned.back().data();
        t.nbytes = ne * 4;
    } else {
        static const uint64_t esz[4] = {4, 2, 4, 8};
        if (__builtin_mul_overflow(ne, esz[t.dtype], &t.nbytes) || t.nbytes > n - off) {
            Q3_LOG("%s: truncated data", what);
            return false;
        }
        t.data = p + off;
    }
    tensors[name] = t;
    return true;
} catch (const std::exception& e) {
    Q3_LOG("%s: %s", what, e.what());
    return false;
}

bool Pack::add_npy(const char* path, const std::string& name) {
    size_t n = 0;
    const uint8_t* p = map_file(path, &n);
    if (!p) {
        Q3_LOG("cannot open %s", path);
        return false;
    }
    return add_npy_bytes(p, n, name, path);
}

bool Pack::add_npz(const char* path, std::string (*rename)(const std::string&)) {
    size_t n = 0;
    const uint8_t* p = map_file(path, &n);
    if (!p) {
        Q3_LOG("cannot open %s as a zip archive", path);
        return false;
    }
    return add_npz_bytes(p, n, path, rename);
}

// Zip: end-of-central-directory record -> central directory -> local headers.  Sizes come from the
// central directory (numpy writes zip64 extras into the local headers with force_zip64=True).
// Every offset and length in the archive is the file's word: `have(o, k)` is asked before bytes [o, o + k) are read.
bool Pack::add_npz_bytes(const uint8_t* p, size_t n, const char* path, std::string (*rename)(const std::string&)) try {
    if (n < 22) {
        Q3_LOG("cannot open %s as a zip archive", path);
        return false;
    }
    auto have = [&](uint64_t o, uint64_t k) { return o <= n && k <= n - o; };
    auto u16 = [&](size_t o) { return (uint32_t)p[o] | ((uint32_t)p[o + 1] << 8); };
    auto u32 = [&](size_t o) { return u16(o) | (u16(o + 2) << 16); };
    auto u64 = [&](size_t o) { return (uint64_t)u32(o) | ((uint64_t)u32(o + 4) << 32); };
    size_t eocd = std::string::npos;
    for (size_t i = n - 22;; i--) {   // [i, i + 22) is inside the file
        if (u32(i) == 0x06054b50u) {
            eocd = i;
            break;
        }
        if (i == 0 || n - i > 22 + 65535) break;
    }
    if (eocd == std::string::npos) {
        Q3_LOG("%s: no zip end-of-central-directory record", path);
        return false;
    }
    uint64_t n_ent = u16(eocd + 10), cd_off = u32(eocd + 16);
    if ((n_ent == 0xffff || cd_off == 0xffffffffu) && eocd >= 20 && u32(eocd - 20) == 0x07064b50u) {
        const uint64_t z64 = u64(eocd - 20 + 8);   // zip64 EOCD locator -> zip64 EOCD record
        if (!have(z64, 56) || u32(z64) != 0x06064b50u) {
            Q3_LOG("%s: the zip64 locator points at no zip64 end-of-central-directory record", path);
            return false;
        }
        n_ent = u64(z64 + 32);
        cd_off = u64(z64 + 48);
    }
    uint64_t c = cd_off;
    int added = 0;
    for (uint64_t e = 0; e < n_ent; e++) {   // every entry takes >= 46 bytes of the file: this ends
        if (!have(c, 46) || u32(c) != 0x02014b50u) {
            Q3_LOG("%s: corrupt zip central directory", path);
            return false;
        }
        const uint32_t method = u16(c + 10), nlen = u16(c + 28), xlen = u16(c + 30), clen = u16(c + 32);
        uint64_t csize = u32(c + 20), usize = u32(c + 24), lho = u32(c + 42);
        if (!have(c + 46, (uint64_t)nlen + xlen + clen)) {
            Q3_LOG("%s: a central directory entry runs past the end of the archive", path);
            return false;
        }
        const std::string member((const char*)p + c + 46, nlen);
        // zip64 extended information (header id 1): only the fields that overflowed, in this order
        const uint64_t xend = c + 46 + nlen + xlen;
        for (uint64_t x = c + 46 + nlen; x + 4 <= xend;) {
            const uint32_t id = u16(x), sz = u16(x + 2);
            if (sz > xend - (x + 4)) {
                Q3_LOG("%s: corrupt extra field of %s", path, member.c_str());
                return false;
            }
            if (id == 1) {
                uint64_t q = x + 4;
                if (usize == 0xffffffffu && q + 8 <= x + 4 + sz) { usize = u64(q); q += 8; }
                if (csize == 0xffffffffu && q + 8 <= x + 4 + sz) { csize = u64(q); q += 8; }
                if (lho == 0xffffffffu && q + 8 <= x + 4 + sz) { lho = u64(q); q += 8; }
            }
            x += 4 + sz;
        }
        c = xend + clen;
        if (!ends_with(member, ".npy")) continue;
        const std::string name = rename(member.substr(0, member.size() - 4));
        if (name.empty()) continue;
        if (!have(lho, 30) || u32(lho) != 0x04034b50u) {
            Q3_LOG("%s: corrupt local header of %s", path, member.c_str());
            return false;
        }
        const uint64_t data = lho + 30 + u16(lho + 26) + u16(lho + 28);   // lho <= n: no wrap
        if (!have(data, csize)) {
            Q3_LOG("%s: member %s runs past the end of the archive", path, member.c_str());
            return false;
        }
        const std::string what = std::string(path) + ":" + member;
        if (method == 0) {
            if (!add_npy_bytes(p + data, (size_t)csize, name, what.c_str())) return false;
        } else if (method == 8) {
            // Deflate's densest code is a 258-byte match in 2 bits: it cannot make more than 1032 bytes from one (zlib's
            // own figure).  Anything above is a damaged directory, and is refused before it is allocated.
            if (usize / 1032 > csize) {
                Q3_LOG("%s: claims %llu bytes from %llu deflated ones", what.c_str(), (unsigned long long)usize,
                       (unsigned long long)csize);
                return false;
            }
            owned.emplace_back((size_t)usize);
            std::vector<uint8_t>& buf = owned.back();
            z_stream zs;
            memset(&zs, 0, sizeof(zs));
            if (inflateInit2(&zs, -MAX_WBITS) != Z_OK) return false;
            zs.next_in = (Bytef*)(p + data);
            zs.next_out = buf.data();
            uint64_t in_left = csize, out_left = usize;
            int rc = Z_OK;
            while (rc == Z_OK) {   // avail_* are 32-bit: feed in slices
                zs.avail_in = (uInt)(in_left > (1u << 30) ? (1u << 30) : in_left);
                zs.avail_out = (uInt)(out_left > (1u << 30) ? (1u << 30) : out_left);
                const uInt ai = zs.avail_in, ao = zs.avail_out;
                rc = inflate(&zs, Z_NO_FLUSH);
                in_left -= ai - zs.avail_in;
                out_left -= ao - zs.avail_out;
                if (rc == Z_OK && ai == zs.avail_in && ao == zs.avail_out) break;
            }
            inflateEnd(&zs);
            if (rc != Z_STREAM_END || out_left != 0) {
                Q3_LOG("%s: inflate failed (%d)", what.c_str(), rc);
                return false;
            }
            if (!add_npy_bytes(buf.data(), buf.size(), name, what.c_str())) return false;
        } else {
            Q3_LOG("%s: zip method %u is not supported (stored and deflate are)", what.c_str(), method);
            return false;
        }
        added++;
    }
    return added > 0;
} catch (const std::exception& e) {
    Q3_LOG("%s: %s", path, e.what());
    return false;
}

bool Pack::add_safetensors(const char* path, std::string (*rename)(const std::string&)) {
    size_t n = 0;
    const uint8_t* p = map_file(path, &n);
    if (!p) {
        Q3_LOG("cannot open %s", path);
        return false;
    }
    return add_safetensors_bytes(p, n, path, rename);
}

bool Pack::add_safetensors_bytes(const uint8_t* p, size_t n, const char* path, std::string (*rename)(const std::string&)) try {
    if (n < 8) {
        Q3_LOG("cannot open %s", path);
        return false;
    }
    uint64_t hlen;
    memcpy(&hlen, p, 8);
    if (hlen > n - 8 || hlen < 2) {
        Q3_LOG("%s: bad safetensors header length", path);
        return false;
    }
    JParser j{(const char*)p + 8, (const char*)p + 8 + hlen};
    const uint8_t* base = p + 8 + hlen;
    const uint64_t avail = n - 8 - hlen;
    if (!j.eat('{')) {
        Q3_LOG("%s: safetensors header is not a JSON object", path);
        return false;
    }
    int added = 0;
    while (j.ok && !j.eat('}')) {
        const std::string key = j.str();
        if (!j.eat(':')) {
            j.ok = false;
            break;
        }
        if (key == "__metadata__") {
            j.skip_value();
        } else {
            JTensor jt;
            if (!j.tensor(jt)) {
                j.ok = false;
                break;
            }
            // The code predictor's first op (scripts/export_code_predictor_onnx.py:38-41): talker hidden -> predictor
            // hidden.  Identity -- no tensors -- for the 0.6 B model whose two widths are both 1024
            // (export_code_predictor_weights.py:51-74 carries none); a checkpoint that DOES hold it is a model this
            // build has no op for, and dropping the tensor would compute something else silently.
            if (key.find("small_to_mtp_projection") != std::string::npos) {
                Q3_LOG("%s: tensor %s: this checkpoint has a talker -> code-predictor projection (small_to_mtp_projection); "
                       "only the identity form (Qwen3-TTS 0.6B: both widths 1024) is built -- refusing to ignore it", path, key.c_str());
                return false;
            }
            const std::string name = rename(key);
            if (!name.empty()) {
                PackTensor t;
                t.name = name;
                if (jt.dtype == "F32") t.dtype = F32;
                else if (jt.dtype == "F16") t.dtype = F16;
                else if (jt.dtype == "BF16") t.dtype = BF16;
                else {
                    Q3_LOG("%s: tensor %s has dtype %s (F32, F16, BF16 are supported)", path, key.c_str(), jt.dtype.c_str());
                    return false;
                }
                if (jt.shape.size() > 4 || jt.end < jt.begin || jt.end > avail) {
                    Q3_LOG("%s: tensor %s: bad shape / offsets", path, key.c_str());
                    return false;
                }
                t.ndim = (uint32_t)jt.shape.size();
                for (size_t d = 0; d < jt.shape.size(); d++) t.shape[d] = jt.shape[d];
                t.nbytes = jt.end - jt.begin;
                uint64_t ne, want;
                if (!t.numel_checked(&ne) || __builtin_mul_overflow(ne, (uint64_t)(t.dtype == F32 ? 4 : 2), &want) || t.nbytes != want) {
                    Q3_LOG("%s: tensor %s: size does not match its shape", path, key.c_str());
                    return false;
                }
                t.data = base + jt.begin;
                tensors[name] = t;
                added++;
            }
        }
        j.eat(',');
    }
    if (!j.ok) {
        Q3_LOG("%s: malformed safetensors header", path);
        return false;
    }
    return added > 0;
} catch (const std::exception& e) {
    Q3_LOG("%s: %s", path, e.what());
    return false;
}

// ---- GGUF (v2 / v3, little-endian): the talker file the reference's server is started with ----------------------
// llama.cpp's qwen3 tensor names -> container names.  Q and K are taken as stored: the converter does not permute them for
// qwen3 (NEOX rope = the rotate-half pairing of DESIGN.md 2).
std::string map_gguf_key(const std::string& k) {
    static const char* const kGgufParts[11] = {"attn_norm", "attn_q", "attn_k", "attn_v", "attn_output", "attn_q_norm",
                                               "attn_k_norm", "ffn_norm", "ffn_gate", "ffn_up", "ffn_down"};
    if (k == "output_norm.weight") return "talker.norm";
    if (k == "token_embd.weight") return "talker.codec_embedding";
    if (k == "output.weight") return "talker.codec_head";
    if (k.compare(0, 4, "blk.") != 0) return "";
    size_t nx = 4;
    while (nx < k.size() && k[nx] >= '0' && k[nx] <= '9') nx++;
    if (nx == 4 || nx - 4 > 6 || nx >= k.size() || k[nx] != '.') return "";   // (a layer number of <= 6 digits: no overflow)
    const int i = atoi(k.c_str() + 4);
    const std::string rest = k.substr(nx + 1);
    for (int p = 0; p < 11; p++)
        if (rest == std::string(kGgufParts[p]) + ".weight") return "talker.layers." + std::to_string(i) + "." + kLayerParts[p];
    return "";
}

namespace {

// A cursor over [p, p + n): every read says whether its bytes were there.
struct GgufCursor {
    const uint8_t* p;
    size_t n, o = 0;
    bool have(uint64_t k) const { return k <= n - o; }   // o <= n always
    template <class T>
    bool get(T* v) {
        if (!have(sizeof(T))) return false;
        memcpy(v, p + o, sizeof(T));
        o += sizeof(T);
        return true;
    }
    bool str(std::string* s) {   // u64 length + bytes
        uint64_t len;
        if (!get(&len) || !have(len)) return false;
        if (s) s->assign((const char*)p + o, (size_t)len);
        o += (size_t)len;
        return true;
    }
};

// size of a scalar GGUF value type, 0 for string / array / unknown
size_t gguf_scalar_size(uint32_t t) {
    static const size_t sz[13] = {1, 1, 2, 2, 4, 4, 4, 1, 0, 0, 8, 8, 8};
    return t < 13 ? sz[t] : 0;
}

// a scalar value as a double (exact for everything this reader looks at); false when its bytes are not there
bool gguf_scalar(GgufCursor& c, uint32_t t, double* out) {
    switch (t) {
        case 0: { uint8_t v; if (!c.get(&v)) return false; *out = v; return true; }
        case 1: { int8_t v; if (!c.get(&v)) return false; *out = v; return true; }
        case 2: { uint16_t v; if (!c.get(&v)) return false; *out = v; return true; }
        case 3: { int16_t v; if (!c.get(&v)) return false; *out = v; return true; }
        case 4: { uint32_t v; if (!c.get(&v)) return false; *out = v; return true; }
        case 5: { int32_t v; if (!c.get(&v)) return false; *out = v; return true; }
        case 6: { float v; if (!c.get(&v)) return false; *out = v; return true; }
        case 7: { uint8_t v; if (!c.get(&v)) return false; *out = v != 0; return true; }
        case 10: { uint64_t v; if (!c.get(&v)) return false; *out = (double)v; return true; }
        case 11: { int64_t v; if (!c.get(&v)) return false; *out = (double)v; return true; }
        case 12: { double v; if (!c.get(&v)) return false; *out = v; return true; }
    }
    return false;
}

const char* ggml_type_name(uint32_t t) {
    static const char* const names[40] = {"F32", "F16", "Q4_0", "Q4_1", "(removed Q4_2)", "(removed Q4_3)", "Q5_0", "Q5_1", "Q8_0", "Q8_1",
                                          "Q2_K", "Q3_K", "Q4_K", "Q5_K", "Q6_K", "Q8_K", "IQ2_XXS", "IQ2_XS", "IQ3_XXS", "IQ1_S",
                                          "IQ4_NL", "IQ3_S", "IQ2_S", "IQ4_XS", "I8", "I16", "I32", "I64", "F64", "IQ1_M",
                                          "BF16", "(removed Q4_0_4_4)", "(removed Q4_0_4_8)", "(removed Q4_0_8_8)", "TQ1_0", "TQ2_0",
                                          "(removed IQ4_NL_4_4)", "(removed IQ4_NL_4_8)", "(removed IQ4_NL_8_8)", "MXFP4"};
    return t < 40 ? names[t] : "unknown";
}

// ggml type -> DType, or -1
int ggml_to_dtype(uint32_t t) {
    switch (t) {
        case 0: return F32;
        case 1: return F16;
        case 30: return BF16;
        case 2: return Q4_0;
        case 8: return Q8_0;
        case 12: return Q4_K;
        case 13: return Q5_K;
        case 14: return Q6_K;
    }
    return -1;
}

}  // namespace

bool Pack::add_gguf(const char* path, std::string (*rename)(const std::string&)) {
    size_t n = 0;
    const uint8_t* p = map_file(path, &n);
    if (!p) {
        Q3_LOG("cannot open %s", path);
        return false;
    }
    return add_gguf_bytes(p, n, path, rename);
}

bool Pack::add_gguf_bytes(const uint8_t* p, size_t n, const char* path, std::string (*rename)(const std::string&)) try {
    GgufCursor c{p, n};
    uint32_t magic = 0, version = 0;
    uint64_t n_tensors = 0, n_kv = 0;
    if (!c.get(&magic) || memcmp(&magic, "GGUF", 4) != 0) {
        Q3_LOG("%s: not a GGUF file (bad magic)", path);
        return false;
    }
    if (!c.get(&version) || (version != 2 && version != 3)) {
        Q3_LOG("%s: GGUF version %u is not supported (2 and 3, little-endian, are)", path, version);
        return false;
    }
    if (!c.get(&n_tensors) || !c.get(&n_kv)) {
        Q3_LOG("%s: truncated GGUF header", path);
        return false;
    }
    // every KV takes >= 12 bytes and every tensor info >= 28: counts the file cannot hold are refused before any loop
    if (n_kv > (n - c.o) / 12 || n_tensors > (n - c.o) / 28) {
        Q3_LOG("%s: GGUF header claims %llu key/value pairs and %llu tensors, more than the file can hold", path,
               (unsigned long long)n_kv, (unsigned long long)n_tensors);
        return false;
    }
    // the keys read: "<arch>.<suffix>" -> the container's meta key
    static const char* const kMetaKeys[8][2] = {{"qwen3.block_count", "talker_layers"},
                                                {"qwen3.embedding_length", "hidden"},
                                                {"qwen3.feed_forward_length", "talker_ffn"},
                                                {"qwen3.attention.head_count", "n_heads"},
                                                {"qwen3.attention.head_count_kv", "n_kv_heads"},
                                                {"qwen3.attention.layer_norm_rms_epsilon", "rms_eps"},
                                                {"qwen3.rope.freq_base", "rope_theta"},
                                                {"qwen3.attention.key_length", "head_dim"}};
    std::map<std::string, double> found;
    double alignment = 32;
    bool have_arch = false;
    for (uint64_t i = 0; i < n_kv; i++) {
        std::string key;
        uint32_t type;
        if (!c.str(&key) || !c.get(&type)) {
            Q3_LOG("%s: GGUF key/value %llu runs past the end of the file", path, (unsigned long long)i);
            return false;
        }
        bool ok = true;
        if (type == 8) {
            std::string v;
            ok = c.str(&v);
            if (ok && key == "general.architecture") {
                have_arch = true;
                if (v != "qwen3") {
                    Q3_LOG("%s: general.architecture is \"%.40s\"; this library reads the qwen3 talker only", path, v.c_str());
                    return false;
                }
            }
        } else if (type == 9) {   // arrays (the tokenizer's) are stepped over, inside the file
            uint32_t et;
            uint64_t cnt;
            ok = c.get(&et) && c.get(&cnt);
            if (ok && et == 9) {
                Q3_LOG("%s: GGUF key %.60s is an array of arrays (not supported)", path, key.c_str());
                return false;
            }
            if (ok && et == 8) {
                for (uint64_t e = 0; e < cnt && ok; e++) ok = c.str(nullptr);   // >= 8 bytes each: this ends
            } else if (ok) {
                const size_t es = gguf_scalar_size(et);
                if (!es) {
                    Q3_LOG("%s: GGUF key %.60s has element type %u (unknown)", path, key.c_str(), et);
                    return false;
                }
                ok = cnt <= (n - c.o) / es;
                if (ok) c.o += (size_t)cnt * es;
            }
        } else {
            double v;
            if (!gguf_scalar_size(type)) {
                Q3_LOG("%s: GGUF key %.60s has value type %u (unknown)", path, key.c_str(), type);
                return false;
            }
            ok = gguf_scalar(c, type, &v);
            if (ok && key == "general.alignment") alignment = v;
            for (const auto& mk : kMetaKeys)
                if (ok && key == mk[0]) found[mk[1]] = v;
        }
        if (!ok) {
            Q3_LOG("%s: the value of GGUF key %.60s runs past the end of the file", path, key.c_str());
            return false;
        }
    }
    if (!have_arch) {
        Q3_LOG("%s: GGUF lacks general.architecture (qwen3 is read)", path);
        return false;
    }
    if (!(alignment >= 8 && alignment <= 1048576) || alignment != (double)(uint64_t)alignment ||
        ((uint64_t)alignment & ((uint64_t)alignment - 1))) {
        Q3_LOG("%s: general.alignment %g is not a power of two >= 8", path, alignment);
        return false;
    }
    const uint64_t align = (uint64_t)alignment;
    // what the kernels are built for (ModelCfg): other values are an unsupported model, like any unsupported geometry
    if (found.count("rope_theta") && found["rope_theta"] != 1e6) {
        Q3_LOG("%s: qwen3.rope.freq_base %g is not the 1e6 this build's RoPE tables are made for", path, found["rope_theta"]);
        return false;
    }
    if (found.count("rms_eps") && (float)found["rms_eps"] != 1e-6f) {
        Q3_LOG("%s: qwen3.attention.layer_norm_rms_epsilon %g is not the 1e-6 this build computes with", path, found["rms_eps"]);
        return false;
    }
    struct Info {
        std::string raw;
        uint32_t ggml = 0;
        PackTensor t;
    };
    std::vector<Info> infos;
    std::map<std::string, int> seen;
    for (uint64_t i = 0; i < n_tensors; i++) {
        Info in;
        uint32_t nd, type;
        uint64_t ne[4] = {1, 1, 1, 1};
        if (!c.str(&in.raw) || !c.get(&nd)) {
            Q3_LOG("%s: GGUF tensor info %llu runs past the end of the file", path, (unsigned long long)i);
            return false;
        }
        if (nd < 1 || nd > 4) {
            Q3_LOG("%s: tensor %.80s has %u dimensions (1..4 are read)", path, in.raw.c_str(), nd);
            return false;
        }
        bool ok = true;
        for (uint32_t d = 0; d < nd && ok; d++) ok = c.get(&ne[d]);
        ok = ok && c.get(&type) && c.get(&in.t.offset);
        if (!ok) {
            Q3_LOG("%s: GGUF tensor info of %.80s runs past the end of the file", path, in.raw.c_str());
            return false;
        }
        if (seen[in.raw]++) {
            Q3_LOG("%s: tensor %.80s appears twice", path, in.raw.c_str());
            return false;
        }
        const int dt = ggml_to_dtype(type);
        if (dt < 0) {
            Q3_LOG("%s: tensor %.80s has ggml type %u (%s); F32, F16, BF16, Q4_0, Q8_0, Q4_K, Q5_K, Q6_K are read", path,
                   in.raw.c_str(), type, ggml_type_name(type));
            return false;
        }
        in.ggml = type;
        in.t.dtype = (uint32_t)dt;
        in.t.ndim = nd;
        for (uint32_t d = 0; d < nd; d++) in.t.shape[d] = ne[nd - 1 - d];   // ne[0] is the innermost: row-major order
        const BlockGeom g = block_geom(in.t.dtype);
        uint64_t numel;
        if (!in.t.numel_checked(&numel) || ne[0] % g.elems ||
            __builtin_mul_overflow(numel / g.elems, (uint64_t)g.bytes, &in.t.nbytes)) {
            Q3_LOG("%s: tensor %.80s: its dimensions overflow, or the row length %llu is no multiple of the %u-element block", path,
                   in.raw.c_str(), (unsigned long long)ne[0], g.elems);
            return false;
        }
        if (in.t.offset % align) {
            Q3_LOG("%s: tensor %.80s: offset %llu is not aligned to %llu", path, in.raw.c_str(), (unsigned long long)in.t.offset,
                   (unsigned long long)align);
            return false;
        }
        infos.push_back(std::move(in));
    }
    const uint64_t data0 = (c.o + align - 1) / align * align;   // c.o <= n and align <= 2^20: no wrap
    int added = 0;
    for (Info& in : infos) {
        PackTensor& t = in.t;
        if (data0 > n || t.offset > n - data0 || t.nbytes > n - data0 - t.offset) {
            Q3_LOG("%s: tensor %.80s runs past the end of the file", path, in.raw.c_str());
            return false;
        }
        const std::string name = rename(in.raw);
        if (name.empty()) continue;
        if (is_block_dtype(t.dtype) && t.ndim != 2) {
            Q3_LOG("%s: tensor %.80s is %s with %u dimensions (a quantised tensor of this model is a matrix)", path, in.raw.c_str(),
                   ggml_type_name(in.ggml), t.ndim);
            return false;
        }
        t.name = name;
        t.data = p + data0 + t.offset;
        t.offset += data0;
        tensors[name] = t;
        added++;
    }
    if (!added) {
        Q3_LOG("%s: no tensor of the qwen3 talker in this GGUF", path);
        return false;
    }
    // tied embeddings: no output.weight -> the head is token_embd
    if (!tensors.count("talker.codec_head") && tensors.count("talker.codec_embedding")) {
        PackTensor t = tensors["talker.codec_embedding"];
        t.name = "talker.codec_head";
        tensors[t.name] = t;
    }
    // geometry comes from the tensors; metadata that contradicts them is a damaged or foreign file
    auto dim = [&](const char* nm, uint32_t d) -> double {
        const PackTensor* t = find(nm);
        return t && d < t->ndim ? (double)t->shape[d] : -1;
    };
    int layers = 0;
    while (tensors.count("talker.layers." + std::to_string(layers) + ".q_proj")) layers++;
    const double hd = found.count("head_dim") ? found["head_dim"] : -1;
    const struct {
        const char* key;
        double have;
        bool comparable;
    } checks[] = {{"talker_layers", (double)layers, layers > 0},
                  {"hidden", dim("talker.layers.0.q_proj", 1), dim("talker.layers.0.q_proj", 1) >= 0},
                  {"talker_ffn", dim("talker.layers.0.gate_proj", 0), dim("talker.layers.0.gate_proj", 0) >= 0},
                  {"head_dim", dim("talker.layers.0.q_norm", 0), dim("talker.layers.0.q_norm", 0) >= 0},
                  {"n_heads", hd > 0 ? dim("talker.layers.0.q_proj", 0) / hd : -1, hd > 0 && dim("talker.layers.0.q_proj", 0) >= 0},
                  {"n_kv_heads", hd > 0 ? dim("talker.layers.0.k_proj", 0) / hd : -1, hd > 0 && dim("talker.layers.0.k_proj", 0) >= 0}};
    for (const auto& ck : checks)
        if (ck.comparable && found.count(ck.key) && found[ck.key] != ck.have) {
            Q3_LOG("%s: GGUF metadata says %s = %g, the tensors say %g", path, ck.key, found[ck.key], ck.have);
            return false;
        }
    for (const auto& kv : found) meta[kv.first] = kv.second;
    meta["gguf_version"] = version;
    meta["gguf_alignment"] = alignment;
    return true;
} catch (const std::exception& e) {
    Q3_LOG("%s: %s", path, e.what());
    return false;
}

// A Q3TTSW1 container, or the reference's deployed files: `path` may be a container file, a
// .safetensors / .npz / .gguf file, or a directory holding model.safetensors (or, without one, exactly one *.gguf) and/or
// code_predictor_weights.npz; `aux_dir` (the servers' --embeddings_dir) adds codec_embedding.npy /
// codec_head.npy and the text front-end's text_embedding / text_projection_* files.  Geometry (layer counts, vocabularies) is taken from what was found.
bool Pack::open_auto(const char* path, const char* aux_dir) {
    // the reference's embeddings/ directory (scripts/extract_embeddings.py:47-66; loaded by
    // llamacpp_talker_server.py:79-93): codec tables + the text front-end's table and projection MLP
    static const char* const kNpyTables[7][2] = {{"codec_embedding.npy", "talker.codec_embedding"},
                                                 {"codec_head.npy", "talker.codec_head"},
                                                 {"text_embedding.npy", "text.embedding"},
                                                 {"text_projection_linear_fc1_weight.npy", "text.fc1.weight"},
                                                 {"text_projection_linear_fc1_bias.npy", "text.fc1.bias"},
                                                 {"text_projection_linear_fc2_weight.npy", "text.fc2.weight"},
                                                 {"text_projection_linear_fc2_bias.npy", "text.fc2.bias"}};
    struct stat st;
    if (!path || stat(path, &st) != 0) {
        Q3_LOG("cannot open %s", path ? path : "(null)");
        return false;
    }
    bool from_gguf = false;   // the talker's tables came out of a GGUF: quantised copies, which exact .npy tables replace
    auto try_file = [&](const std::string& f) -> int {   // 1 added, 0 absent, -1 error
        struct stat s2;
        if (stat(f.c_str(), &s2) != 0 || !S_ISREG(s2.st_mode)) return 0;
        if (ends_with(f, ".safetensors")) return add_safetensors(f.c_str(), map_safetensors_key) ? 1 : -1;
        if (ends_with(f, ".npz")) return add_npz(f.c_str(), map_cp_npz_key) ? 1 : -1;
        if (ends_with(f, ".gguf")) {
            from_gguf = true;
            return add_gguf(f.c_str(), map_gguf_key) ? 1 : -1;
        }
        return 0;
    };
    auto try_npy = [&](const std::string& dir, const char* file, const char* name) -> int {
        const std::string f = dir + "/" + file;
        struct stat s2;
        const bool over_gguf = from_gguf && (!strcmp(name, "talker.codec_embedding") || !strcmp(name, "talker.codec_head"));
        if ((tensors.count(name) && !over_gguf) || stat(f.c_str(), &s2) != 0) return 0;
        if (over_gguf && tensors.count(name)) {
            // the reference applies the .npy head in Python (llamacpp_talker_server.py:79-93): the exact table, not the
            // GGUF's quantised token_embd / output
            Q3_LOG("%s: taken from %s, not from the GGUF's quantised copy", name, f.c_str());
            tensors.erase(name);
        }
        return add_npy(f.c_str(), name) ? 1 : -1;
    };
    auto begins_with_gguf_magic = [](const char* f) {
        char m[4] = {0, 0, 0, 0};
        FILE* fp = fopen(f, "rb");
        if (!fp) return false;
        const bool is = fread(m, 1, 4, fp) == 4 && memcmp(m, "GGUF", 4) == 0;
        fclose(fp);
        return is;
    };
    int found = 0;
    if (S_ISREG(st.st_mode)) {
        const std::string f(path);
        if (ends_with(f, ".gguf") || begins_with_gguf_magic(path)) {
            from_gguf = true;
            if (!add_gguf(path, map_gguf_key)) return false;
            found++;
        } else {
            if (!ends_with(f, ".safetensors") && !ends_with(f, ".npz")) return open(path);
            const int r = try_file(f);
            if (r < 0) return false;
            found += r;
        }
    } else if (S_ISDIR(st.st_mode)) {
        const std::string d(path);
        for (const char* f : {"model.safetensors", "code_predictor_weights.npz"}) {
            const int r = try_file(d + "/" + f);
            if (r < 0) return false;
            found += r;
        }
        struct stat s2;
        if (stat((d + "/model.safetensors").c_str(), &s2) != 0) {   // a deployment that holds only the talker's GGUF
            std::vector<std::string> ggufs;
            if (DIR* dh = opendir(path)) {
                while (const dirent* e = readdir(dh))
                    if (ends_with(e->d_name, ".gguf")) ggufs.push_back(e->d_name);
                closedir(dh);
            }
            if (ggufs.size() > 1) {
                Q3_LOG("%s holds %zu .gguf files (%s, %s, ...): name the talker's file itself", path, ggufs.size(), ggufs[0].c_str(),
                       ggufs[1].c_str());
                return false;
            }
            if (ggufs.size() == 1) {
                const int r = try_file(d + "/" + ggufs[0]);
                if (r < 0) return false;
                found += r;
            }
        }
        for (const auto& e : kNpyTables) {
            const int r = try_npy(d, e[0], e[1]);
            if (r < 0) return false;
            found += r;
        }
    }
    if (aux_dir && *aux_dir) {
        for (const auto& e : kNpyTables) {
            const int r = try_npy(aux_dir, e[0], e[1]);
            if (r < 0) return false;
            found += r;
        }
    }
    if (!found) {
        Q3_LOG("%s: no Q3TTSW1 container, model.safetensors, talker .gguf or code_predictor_weights.npz found", path);
        return false;
    }
    // geometry from the tensors: layers present, vocabulary rows (the re-keyed talker pads both
    // tables to the text vocabulary: only the codec rows are used, scripts/extract_talker_as_qwen3.py:57-69)
    auto count_layers = [&](const char* stack) {
        int nl = 0;
        while (tensors.count(std::string(stack) + ".layers." + std::to_string(nl) + ".q_proj")) nl++;
        return nl;
    };
    const int tl = count_layers("talker"), cl = count_layers("cp");
    if (tl) meta["talker_layers"] = tl;
    if (cl) meta["cp_layers"] = cl;
    int groups = 0;
    while (tensors.count("cp.lm_head." + std::to_string(groups))) groups++;
    if (groups) meta["cp_groups"] = groups;
    const int talker_vocab = 3072;
    for (const char* nm : {"talker.codec_embedding", "talker.codec_head"}) {
        auto it = tensors.find(nm);
        if (it != tensors.end() && it->second.ndim == 2 && it->second.shape[0] > (uint64_t)talker_vocab) {
            PackTensor& t = it->second;
            t.nbytes = t.nbytes / t.shape[0] * talker_vocab;
            t.shape[0] = talker_vocab;
        }
    }
    if (const PackTensor* g = find("talker.layers.0.gate_proj")) meta["talker_ffn"] = (double)g->shape[0];
    if (const PackTensor* g = find("cp.layers.0.gate_proj")) meta["cp_ffn"] = (double)g->shape[0];
    return true;
}

}  // namespace q3
