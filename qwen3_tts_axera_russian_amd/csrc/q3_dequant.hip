// q3_dequant.hip -- ggml block formats (Q4_0, Q8_0, Q4_K, Q5_K, Q6_K) -> row-major fp16 or fp32, at load time.
//
// The fp32 value of an element is the one ggml's dequantize_row_* produces ("GGUF"): every product below
// is exact in fp32 (operand widths sum to <= 24 bits), the K-quants' one subtraction is the one rounding, so an FMA
// contraction cannot change a bit.  The fp16 output is that value rounded to nearest even with saturation at +-65504
// (f2h_sat's rule); the f32 output is the value itself.
//
// One thread makes 8 consecutive outputs -- one 16-byte store of fp16, two of fp32.  A block's K is a multiple of 32
// and 8 divides 32, so a thread's outputs share one block, one 32-element sub-block and so one scale and one minimum,
// unpacked once.  Blocks are 18 / 34 / 144 / 176 / 210 bytes: nothing wider than a byte is aligned in all of them, so
// the quants are read with byte loads (consecutive threads read consecutive bytes; this runs once per tensor at load).
#include "q3_model.h"

namespace q3 {

namespace {

__device__ inline float ld_f16(const uint8_t* p, int* bad) {
    const uint32_t u = (uint32_t)p[0] | ((uint32_t)p[1] << 8);
    if ((u & 0x7c00u) == 0x7c00u) *bad = 1;   // Inf / NaN scale: ggml's validation rejects such a file
    _Float16 h;
    const uint16_t v = (uint16_t)u;
    __builtin_memcpy(&h, &v, 2);
    return (float)h;
}

// 6-bit scale and minimum j (0..7) of a K-quant's 12 packed bytes
__device__ inline void scale_min_k4(int j, const uint8_t* s, int* sc, int* m) {
    if (j < 4) {
        *sc = s[j] & 63;
        *m = s[j + 4] & 63;
    } else {
        *sc = (s[j + 4] & 15) | ((s[j - 4] >> 6) << 4);
        *m = (s[j + 4] >> 4) | ((s[j] >> 6) << 4);
    }
}

// v[0..8) = elements e .. e+7 (e % 8 == 0) of the block at b
template <int TYPE>
__device__ inline void dequant8(const uint8_t* b, int e, float* v, int* bad) {
    if constexpr (TYPE == Q8_0) {
        const float d = ld_f16(b, bad);
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = d * (float)(int8_t)b[2 + e + i];
    } else if constexpr (TYPE == Q4_0) {
        const float d = ld_f16(b, bad);
        const int hi = e >= 16;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int q = b[2 + (e & 15) + i];
            v[i] = d * (float)((hi ? q >> 4 : q & 15) - 8);
        }
    } else if constexpr (TYPE == Q4_K || TYPE == Q5_K) {
        const float d = ld_f16(b, bad), dmin = ld_f16(b + 2, bad);
        const int c = e >> 6, h = (e >> 5) & 1, j = 2 * c + h, l = e & 31;
        int sc, m;
        scale_min_k4(j, b + 4, &sc, &m);
        const float d1 = d * (float)sc, m1 = dmin * (float)m;
        const uint8_t* qs = b + (TYPE == Q5_K ? 48 : 16) + 32 * c + l;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            int q = h ? qs[i] >> 4 : qs[i] & 15;
            if constexpr (TYPE == Q5_K) q += 16 * ((b[16 + l + i] >> j) & 1);
            v[i] = d1 * (float)q - m1;
        }
    } else {   // Q6_K: ql[128] qh[64] sc[16] d
        const float d = ld_f16(b + 208, bad);
        const int c = e >> 7, t = (e >> 5) & 3, l = e & 31;
        const float ds = d * (float)(int8_t)b[192 + 8 * c + (l >> 4) + 2 * t];
        const uint8_t* ql = b + 64 * c + l + 32 * (t & 1);
        const uint8_t* qh = b + 128 + 32 * c + l;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int nib = t < 2 ? ql[i] & 15 : ql[i] >> 4;
            v[i] = ds * (float)((nib | (((qh[i] >> (2 * t)) & 3) << 4)) - 32);
        }
    }
}

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

// n8 = outputs / 8.  Exactly one of out16 / out32 is set.
template <int TYPE, int BLOCK, int BYTES>
__global__ __launch_bounds__(256) void dequant_kernel(const uint8_t* __restrict__ blocks, size_t n8, half_t* __restrict__ out16,
                                                      float* __restrict__ out32, int* __restrict__ flag) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n8) return;
    const size_t E = g * 8;
    float v[8];
    int bad = 0;
    dequant8<TYPE>(blocks + (E / BLOCK) * BYTES, (int)(E % BLOCK), v, &bad);
    if (bad) *flag = 1;   // an ordinary vector store; every writer writes the same value
    if (out16) {
        half8 h;
#pragma unroll
        for (int i = 0; i < 8; i++) h[i] = (_Float16)fminf(fmaxf(v[i], -65504.f), 65504.f);
        *(half8*)(out16 + E) = h;
    } else {
        *(floatx4*)(out32 + E) = floatx4{v[0], v[1], v[2], v[3]};
        *(floatx4*)(out32 + E + 4) = floatx4{v[4], v[5], v[6], v[7]};
    }
}

}  // namespace

int launch_dequant(hipStream_t s, uint32_t type, const uint8_t* blocks, size_t n_rows, size_t K, half_t* out_f16, float* out_f32,
                   int* flag) {
    const BlockGeom g = block_geom(type);
    if (!is_block_dtype(type) || !blocks || !flag || (out_f16 != nullptr) == (out_f32 != nullptr) || K == 0 || K % g.elems) {
        Q3_LOG("launch_dequant: bad arguments (type %u, K %zu)", type, K);
        return -1;
    }
    const size_t n8 = n_rows * K / 8;
    if (n8 == 0) return 0;
    const size_t grid = (n8 + 255) / 256;
    if (grid > 0x7fffffffu) {
        Q3_LOG("launch_dequant: %zu x %zu elements are more than one launch takes", n_rows, K);
        return -1;
    }
#define Q3_DQ(T, B, NB) hipLaunchKernelGGL((dequant_kernel<T, B, NB>), dim3((unsigned)grid), dim3(256), 0, s, blocks, n8, out_f16, out_f32, flag)
    switch (type) {
        case Q4_0: Q3_DQ(Q4_0, 32, 18); break;
        case Q8_0: Q3_DQ(Q8_0, 32, 34); break;
        case Q4_K: Q3_DQ(Q4_K, 256, 144); break;
        case Q5_K: Q3_DQ(Q5_K, 256, 176); break;
        default: Q3_DQ(Q6_K, 256, 210); break;
    }
#undef Q3_DQ
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

}  // namespace q3
