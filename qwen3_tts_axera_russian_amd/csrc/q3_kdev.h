// q3_kdev.h -- what the kernel files (q3_linear.hip, q3_attn.hip, q3_sample.hip, q3_rows.hip) share on the device:
// vector types, the timeline / wave-priority macros, the RMSNorm fold's constants and the row producers.  Device code:
// included by .hip files only.
#pragma once
#include "q3_kernels.h"
#include "q3_xlane.h"   // the cross-lane exchange helpers and the butterflies (shared with q3_spk.hip)
#ifdef Q3_TIMELINE
#include "q3_timeline.h"
#endif

namespace q3 {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));

// ---- diagnostic timeline (only in the -DQ3_TIMELINE build; the product build compiles it away) ----
#ifdef Q3_TIMELINE
#define Q3_TL(id)      \
    if (g_tls.skip) return; \
    TlScope2 tl_scope2_(a.tl_node, id); \
    TlScope tl_scope_(id)
#define Q3_PH(n)                                                                                                   \
    do {                                                                                                           \
        if (tl_scope_.slot < g_tls.cap && g_tls.ph) g_tls.ph[(size_t)tl_scope_.slot * 8 + (n)] = wall_clock64(); \
    } while (0)
#else
// Every kernel of the frame loop (and the prefill) raises its waves' issue priority at entry (s_setprio 3; -DQ3_WAVE_PRIO=0 builds
// without).  Alone on the chip it changes nothing (2.40 ms per frame step either way).  Beside the vocoder's one-workgroup-per-CU
// grid (voc_set_max_workgroups(-1)) a frame-loop wave shares its SIMD with one vocoder wave that issues MFMAs and LDS reads back to
// back; with priority the frame step beside the decode takes 3.0 instead of 3.2 ms and the benchmark's step 211 instead of 232 ms
// (round 2 tried the priority beside an UNCAPPED vocoder grid, where the frame loop's workgroups found no room at all: no effect).
#ifndef Q3_WAVE_PRIO
#define Q3_WAVE_PRIO 3
#endif
#if Q3_WAVE_PRIO > 0
#define Q3_TL(id) __builtin_amdgcn_s_setprio(Q3_WAVE_PRIO)
#else
#define Q3_TL(id)
#endif
#define Q3_PH(n)
#endif

// Kernel arguments passed as one struct live in the kernarg segment and are fetched with scalar loads where the code
// first needs them; behind control flow that becomes a CHAIN of s_load -> s_waitcnt round trips before the first
// global load of a kernel is even issued (six of them in attn_kernel, seen in the ISA).  Naming the scalar fields in
// one empty asm statement at the top makes the compiler fetch them all at once (adjacent fields merge into wide
// loads) and wait once.
#define Q3_FETCH_ARGS(...) asm volatile("" ::__VA_ARGS__)

// A per-row scalar (position, slot, frame counter ...) that a previous kernel wrote and every lane of the workgroup
// needs: read through the constant address space, i.e. with a SCALAR load (s_load_dword: straight into an SGPR, its
// own counter, ~half the latency of a vector load, and the vector loads that follow are issued without waiting for
// it).  Written by an earlier launch only, never by this one: the scalar cache is invalidated at every dispatch.
__device__ __forceinline__ int uniform_load(const int* p) {
    return *(const __attribute__((address_space(4))) int*)p;
}

__device__ __forceinline__ half_t sat_half(float x) {
    return (half_t)fminf(fmaxf(x, -65504.f), 65504.f);
}
// RMSNorm folded around the GEMM (numerics contract): the PRODUCER of a residual row also writes
// xh = fp16((h * gamma_consumer) * NORM_PRE) -- the consumer's norm weight applied, a fixed power-of-two pre-scale
// keeping |h * gamma| up to 1e6 inside fp16 -- and the consumer multiplies its f32 accumulators by
// inv_rms(row) * NORM_POST.  The GEMM reads 2 bytes per activation instead of 4 and has no prologue to wait for.
constexpr float NORM_PRE = 0.0625f, NORM_POST = 16.0f;
// Stores of the decode kernels' outputs (a few hundred KB per launch, read by the NEXT launch on other XCDs): plain.
// -DQ3_NT_OUT makes them non-temporal (written through instead of left dirty for the end-of-kernel write-back) --
// measured in round 3 on MI355X: 2.41 -> 2.49 ms per frame at 32 rows, 2.14 -> 2.20 at one; rejected, kept as a probe.
#ifdef Q3_NT_OUT
#define Q3_OUT_STORE(v_, p_) __builtin_nontemporal_store((v_), (p_))
#else
#define Q3_OUT_STORE(v_, p_) (*(p_) = (v_))
#endif
__device__ __forceinline__ half_t pre_scaled(float h, float g) { return sat_half((h * g) * NORM_PRE); }

// A residual row leaves its producer as: h (f32), 64 sum-of-squares partials, and xh = the consumer's pre-scaled
// fp16 GEMM input (see NORM_PRE); gamma = the consuming layer's norm weight (null: no xh).
__device__ __forceinline__ void store_row_ssq(float* h, float* ssq, int r, int H, int k4, float4 v,
                                              half_t* xh = nullptr, const float* gamma = nullptr) {
    *(float4*)(h + frag_idx(r, k4 * 4, H)) = v;
    if (xh) {
        const float4 g = *(const float4*)(gamma + k4 * 4);
        half_t* p = xh + frag_idx(r, k4 * 4, H);
        p[0] = pre_scaled(v.x, g.x);
        p[1] = pre_scaled(v.y, g.y);
        p[2] = pre_scaled(v.z, g.z);
        p[3] = pre_scaled(v.w, g.w);
    }
    float s = v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    s = group_sum_up<4>(s);   // every caller's k4 loop runs whole quads (H is a multiple of 16)
    if ((k4 & 3) == 0) ssq[(size_t)r * (H / 16) + (k4 >> 2)] = s;
}

// `codes` points at the row's 16 codes; (ov_g, ov_tok) overrides group ov_g with a value the caller
// just computed (no same-kernel global read-after-write).
__device__ __forceinline__ void feedback_row(const int* codes, int r, const float* talker_emb, int talker_vocab,
                                             const float* const* cp_tables, int cp_vocab, int n_groups,
                                             const float* pad, float* h_out, float* ssq_out, int H,
                                             int ov_g = -1, int ov_tok = 0, const int* fz = nullptr,
                                             half_t* xh_out = nullptr, const float* gamma = nullptr) {
    // tts_client.py:199-208: copy codec_embedding[code_0], += cp table g row, += tts_pad, in this order
    // (fz: teacher-forced ids of this frame, tests only -- entries >= 0 replace the recorded decisions)
    int c0 = codes[0];
    if (fz && fz[0] >= 0 && c0 >= 0) c0 = fz[0];
    for (int k4 = threadIdx.x; k4 < H / 4; k4 += blockDim.x) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c0 >= 0 && c0 < talker_vocab) v = *(const float4*)(talker_emb + (size_t)c0 * H + k4 * 4);
        for (int g = 0; g < n_groups; g++) {
            int t = g == ov_g ? ov_tok : codes[1 + g];
            if (fz && g != ov_g && fz[1 + g] >= 0) t = fz[1 + g];
            if (t >= 0 && t < cp_vocab) {
                const float4 e = *(const float4*)(cp_tables[g] + (size_t)t * H + k4 * 4);
                v.x += e.x;
                v.y += e.y;
                v.z += e.z;
                v.w += e.w;
            }
        }
        if (pad) {
            const float4 e = *(const float4*)(pad + k4 * 4);
            v.x += e.x;
            v.y += e.y;
            v.z += e.z;
            v.w += e.w;
        }
        store_row_ssq(h_out, ssq_out, r, H, k4, v, xh_out, gamma);
    }
}

}  // namespace q3
