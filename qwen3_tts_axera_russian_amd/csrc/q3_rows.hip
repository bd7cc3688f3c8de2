// q3_rows.hip -- gfx950 (MI355X, CDNA4) row kernels of the Qwen3-TTS frame loop and its admissions: sum-of-squares
// partials of uploaded rows, the final RMSNorm, prefix-cache moves, embedding gathers, the feedback sum and codec-prompt
// rows.  Wave = 64 lanes.
#include "q3_kdev.h"

namespace q3 {

// ---------------------------------------------------------------------------
// ssq partials of uploaded rows
// ---------------------------------------------------------------------------
__global__ void ssq_rows_kernel(const float* __restrict__ rows, float* __restrict__ h, float* __restrict__ ssq, int H,
                                half_t* __restrict__ xh, const float* __restrict__ gamma, int dst_row0) {
    const int r = blockIdx.x;
    for (int k4 = threadIdx.x; k4 < H / 4; k4 += blockDim.x)
        store_row_ssq(h, ssq, dst_row0 + r, H, k4, *(const float4*)(rows + (size_t)r * H + k4 * 4), xh, gamma);
}
int launch_ssq_rows(hipStream_t s, const float* rows, float* h, float* ssq, int R, int H, half_t* xh, const float* gamma,
                    int dst_row0) {
    if (R <= 0) return 0;
    hipLaunchKernelGGL(ssq_rows_kernel, dim3(R), dim3(256), 0, s, rows, h, ssq, H, xh, gamma, dst_row0);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

// ---------------------------------------------------------------------------
// final RMSNorm of selected rows
// ---------------------------------------------------------------------------
__global__ void final_norm_kernel(FinalNormArgs a) {
    Q3_FETCH_ARGS("s"(a.h), "s"(a.ssq), "s"(a.ssq_parts), "s"(a.gamma), "s"(a.eps), "s"(a.H), "s"(a.row0), "s"(a.row_map), "s"(a.src_off),
                  "s"(a.out_f32), "s"(a.out_f16), "s"(a.out_copy), "s"(a.out_copy_ssq), "s"(a.out_copy_xh), "s"(a.out_copy_gamma),
                  "s"(a.out_copy_row_off));
    Q3_TL(40);
    __shared__ float inv_sh;
    const int r = a.row0 + blockIdx.x;
    const int src = a.row_map ? uniform_load(a.row_map + r) : r + a.src_off;
    if (threadIdx.x < 64) {
        float s = 0.f;
        for (int p = threadIdx.x; p < a.ssq_parts; p += 64) s += a.ssq[(size_t)src * a.ssq_parts + p];
        s = wave_sum(s);
        if (threadIdx.x == 0) inv_sh = 1.0f / sqrtf(s / (float)a.H + a.eps);
    }
    __syncthreads();
    const float iv = inv_sh;
    for (int k4 = threadIdx.x; k4 < a.H / 4; k4 += blockDim.x) {
        const float4 v = *(const float4*)(a.h + frag_idx(src, k4 * 4, a.H));
        const float4 g = *(const float4*)(a.gamma + k4 * 4);
        float4 o;
        o.x = (v.x * iv) * g.x;
        o.y = (v.y * iv) * g.y;
        o.z = (v.z * iv) * g.z;
        o.w = (v.w * iv) * g.w;
        if (a.out_f32) *(float4*)(a.out_f32 + (size_t)r * a.H + k4 * 4) = o;
        if (a.out_f16) {
            half_t* p = a.out_f16 + frag_idx(r, k4 * 4, a.H);
            p[0] = sat_half(o.x);
            p[1] = sat_half(o.y);
            p[2] = sat_half(o.z);
            p[3] = sat_half(o.w);
        }
        if (a.out_copy)
            store_row_ssq(a.out_copy, a.out_copy_ssq, r + a.out_copy_row_off, a.H, k4, o, a.out_copy_xh, a.out_copy_gamma);
    }
}
int launch_final_norm(hipStream_t s, const FinalNormArgs& a) {
    if (a.R <= 0) return 0;
    FinalNormArgs a2 = a;
    a2.tl_node = tl_next_node();
    hipLaunchKernelGGL(final_norm_kernel, dim3(a.R), dim3(256), 0, s, a2);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

// ---------------------------------------------------------------------------
// prefix cache: an utterance's prefix state between its KV slot and a pool entry
// ---------------------------------------------------------------------------
// grid (x, n_layers * 2 * n_kv): workgroups (., y) move run y = (layer, K|V, head), 16 bytes per lane, grid-stride over
// the run; those of run 0 also move the residual row and its ssq partials.
__global__ void __launch_bounds__(256) prefix_move_kernel(PrefixMoveArgs a) {
    const int run = blockIdx.y;
    const int head = run % a.n_kv, kv = (run / a.n_kv) & 1, layer = run / (2 * a.n_kv);
    uint4* cache = (uint4*)((kv ? a.vc : a.kc) + (size_t)layer * a.layer_stride + ((size_t)a.slot * a.n_kv + head) * a.n_ctx * 128);
    uint4* ent = (uint4*)(a.entry + (size_t)run * a.max_rows * 128);
    const uint4* src = a.restore ? ent : cache;
    uint4* dst = a.restore ? cache : ent;
    const int n16 = a.n_rows * 16;   // 16-byte groups of the run
    const int i0 = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
    for (int i = i0; i < n16; i += step) dst[i] = src[i];
    if (run != 0) return;
    for (int k4 = i0; k4 < a.H / 4; k4 += step) {
        float4* ph = (float4*)(a.h + frag_idx(a.h_row, k4 * 4, a.H));
        float4* pe = (float4*)(a.state + k4 * 4);
        if (a.restore) *ph = *pe;
        else *pe = *ph;
    }
    const int parts = a.H / 16;
    for (int p = i0; p < parts; p += step) {
        float* ps = a.ssq + (size_t)a.h_row * parts + p;
        float* pe = a.state + a.H + p;
        if (a.restore) *ps = *pe;
        else *pe = *ps;
    }
}
int launch_prefix_move(hipStream_t s, const PrefixMoveArgs& a) {
    if (!a.kc || !a.vc || !a.entry || !a.state || !a.h || !a.ssq || a.n_layers <= 0 || a.n_kv <= 0 || a.slot < 0 || a.n_rows <= 0 ||
        a.n_rows > a.n_ctx || a.n_rows > a.max_rows || a.h_row < 0 || a.H <= 0 || a.H % 32) {
        Q3_LOG("launch_prefix_move: bad arguments (%d rows, entry of %d, n_ctx %d)", a.n_rows, a.max_rows, a.n_ctx);
        return -1;
    }
    int gx = (a.n_rows * 16 + 255) / 256;   // 256 lanes x 16 B = 16 rows of a run per workgroup
    if (gx > 8) gx = 8;
    hipLaunchKernelGGL(prefix_move_kernel, dim3(gx, a.n_layers * 2 * a.n_kv), dim3(256), 0, s, a);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

// ---------------------------------------------------------------------------
// embedding gather with ssq partials
// ---------------------------------------------------------------------------
__global__ void gather_embed_kernel(const float* __restrict__ table, int V, int H, const int* __restrict__ tok,
                                    int tok_stride, const int* __restrict__ n_frames, int frame_cap, int col,
                                    float* __restrict__ h, float* __restrict__ ssq, int row0, int R_total,
                                    const int* __restrict__ forced, half_t* __restrict__ xh,
                                    const float* __restrict__ gamma) {
    const int r = row0 + blockIdx.x;
    int t;
    if (n_frames) {
        int f = uniform_load(n_frames + r) - 1;
        if (f < 0) f = 0;
        if (f >= frame_cap) f = frame_cap - 1;
        t = uniform_load(tok + ((size_t)f * R_total + r) * 16 + col);
        if (forced) {   // teacher forcing (tests): continue with the forced id where one is given
            const int fz = uniform_load(forced + ((size_t)f * R_total + r) * 16 + col);
            if (fz >= 0 && t >= 0) t = fz;
        }
    } else {
        t = tok[(size_t)r * tok_stride];
    }
    const bool ok = t >= 0 && t < V;
    for (int k4 = threadIdx.x; k4 < H / 4; k4 += blockDim.x) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok) v = *(const float4*)(table + (size_t)t * H + k4 * 4);
        store_row_ssq(h, ssq, r, H, k4, v, xh, gamma);
    }
}
int launch_gather_embed(hipStream_t s, const float* table, int V, int H, const int* tok, int tok_stride,
                        const int* n_frames, int frame_cap, int col, float* h, float* ssq, int R, int row0,
                        int R_total, const int* forced, half_t* xh, const float* gamma) {
    if (R <= 0) return 0;
    hipLaunchKernelGGL(gather_embed_kernel, dim3(R), dim3(256), 0, s, table, V, H, tok, tok_stride, n_frames,
                       frame_cap, col, h, ssq, row0, R_total > 0 ? R_total : R, forced, xh, gamma);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

__global__ void feedback_kernel(const int* codes, const float* talker_emb, int talker_vocab,
                                const float* const* cp_tables, int cp_vocab, int n_groups, const float* pad,
                                float* h_out, float* ssq_out, int H, half_t* xh_out, const float* gamma) {
    feedback_row(codes + (size_t)blockIdx.x * 16, blockIdx.x, talker_emb, talker_vocab, cp_tables, cp_vocab, n_groups,
                 pad, h_out, ssq_out, H, -1, 0, nullptr, xh_out, gamma);
}
int launch_feedback(hipStream_t s, const int* codes16, int R, const float* talker_emb, int talker_vocab,
                    const float* const* cp_tables, int cp_vocab, int n_groups, const float* pad_embed,
                    float* h_out, float* ssq_out, int H, half_t* xh_out, const float* gamma) {
    if (R <= 0) return 0;
    hipLaunchKernelGGL(feedback_kernel, dim3(R), dim3(256), 0, s, codes16, talker_emb, talker_vocab, cp_tables,
                       cp_vocab, n_groups, pad_embed, h_out, ssq_out, H, xh_out, gamma);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

// codec prompt (PromptRowsArgs): workgroup i owns prompt frame i.  The ring and the counter are written with plain vector
// stores by lane 0; every workgroup writes other words, and the frame's sampler reads them in a later launch.
__global__ void __launch_bounds__(256) prompt_rows_kernel(PromptRowsArgs a) {
    const int i = blockIdx.x;
    const int* codes = a.codes + (size_t)i * 16;
    if (threadIdx.x == 0) {
        if (i >= a.T - 32) a.past[i & 31] = codes[0];
        if (i == a.T - 1) a.n_past[0] = a.T;
        // the seen-set takes every frame; workgroups share its words: a vector atomic on global memory
        if (a.seen && codes[0] >= 0 && codes[0] < a.seen_vocab) atomicOr(a.seen + (codes[0] >> 5), 1u << (codes[0] & 31));
    }
    if (a.h)
        feedback_row(codes, a.row0 + i, a.talker_emb, a.talker_vocab, a.cp_tables, a.cp_vocab, a.n_groups, a.pad_embed,
                     a.h, a.ssq, a.H, -1, 0, nullptr, a.xh, a.gamma);
}
int launch_prompt_rows(hipStream_t s, const PromptRowsArgs& a) {
    if (a.T <= 0) return 0;
    if (!a.codes || !a.past || !a.n_past || !a.talker_emb || !a.cp_tables || a.n_groups <= 0 || a.n_groups > 15 ||
        (a.seen && a.seen_vocab <= 0) || (a.h && (!a.ssq || a.row0 < 0 || a.row0 + a.T > a.max_rows || a.H <= 0 || a.H % 16))) {
        Q3_LOG("launch_prompt_rows: bad arguments (%d frames at row %d of %d)", a.T, a.row0, a.max_rows);
        return -1;
    }
    hipLaunchKernelGGL(prompt_rows_kernel, dim3(a.T), dim3(256), 0, s, a);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

}  // namespace q3
