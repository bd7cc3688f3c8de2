// q3_attn.hip -- gfx950 (MI355X, CDNA4) attention kernels of the Qwen3-TTS talker / code predictor.  Wave = 64 lanes.
//
// Hot-path map (reference file:line each kernel stands in for):
//   attn_kernel     per-head q/k RMSNorm + RoPE + KV-cache append + GQA decode
//                   attention (one workgroup per (row, kv head), K/V straight to
//                   VGPRs, scores staged in LDS).
#include "q3_kdev.h"

namespace q3 {

// ---------------------------------------------------------------------------
// attention: one workgroup per (row, kv head).  Phase A (waves 0-3): per-head RMSNorm + RoPE of the
// two q heads and the k head, v pass-through, K/V appended to the cache.  Phase B: every 16-lane
// group walks cached rows t = grp, grp+ngrp, ... (16 B of K and of V per lane, straight to VGPRs)
// with an online softmax per group, groups are merged by shuffles inside a wave and through LDS
// across waves: two barriers in all, no n_ctx-sized LDS.
// ---------------------------------------------------------------------------
template <int MODE, int APRE>
__global__ void __launch_bounds__(1024) attn_kernel(AttnArgs a) {
    constexpr int D = 128;
    Q3_FETCH_ARGS("s"(a.qkv), "s"(a.ld), "s"(a.row0), "s"(a.q_norm), "s"(a.k_norm), "s"(a.eps), "s"(a.rope_cos), "s"(a.rope_sin),
                  "s"(a.slot), "s"(a.pos), "s"(a.slot_base), "s"(a.slot_stride), "s"(a.pos_base), "s"(a.pos_stride), "s"(a.kc),
                  "s"(a.vc), "s"(a.n_ctx), "s"(a.n_kv), "s"(a.n_heads), "s"(a.out), "s"(a.scale), "s"(a.valid_mod), "s"(a.valid_n));
    Q3_TL(30 + MODE);
    const int r = a.row0 + blockIdx.x, g = blockIdx.y;
    if (a.valid_mod > 0 && (r % a.valid_mod) >= a.valid_n) return;   // padding row of a multi-position pass (block-uniform)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int nwv = blockDim.x >> 6;
    const int slot = a.slot ? uniform_load(a.slot + r) : a.slot_base + r * a.slot_stride;
    const int pos = a.pos ? uniform_load(a.pos + r) : a.pos_base + r * a.pos_stride;
    __shared__ float qs[2][D];
    __shared__ float knew[D], vnew[D];
    extern __shared__ __attribute__((aligned(16))) float dyn[];
    float* pm = dyn;                    // [nwv][2]  running max per wave/head
    float* pl = dyn + 2 * nwv;          // [nwv][2]  running sum
    float* pacc = dyn + 4 * nwv;        // [nwv][2][D]
    float* row = a.qkv + (size_t)r * a.ld;
    const size_t cbase = ((size_t)slot * a.n_kv + g) * (size_t)a.n_ctx * D;
    const int T = (MODE == ATTN_FUSED) ? pos : pos + 1;  // rows read from the cache
    const int l16 = tid & 15, grp = tid >> 4, ngrp = blockDim.x >> 4;
    const half_t* kbase = a.kc + cbase;
    const half_t* vbase = a.vc + cbase;

    // ---- all loads of the short-T case are issued here: phase A operands first (consumed first;
    // vmcnt retires in order), then the first APRE cached K/V rows of every group ----
    float x0 = 0.f, x1 = 0.f, gm0 = 1.f, gm1 = 1.f, cs = 1.f, sn = 0.f;
    if (MODE != ATTN_ATTEND && w < 4) {
        // wave 0,1: q heads 2g, 2g+1; wave 2: k head g; wave 3: v head g
        const float* src = w < 2 ? row + (size_t)(2 * g + w) * D
                         : w == 2 ? row + (size_t)(a.n_heads + g) * D
                                  : row + (size_t)(a.n_heads + a.n_kv + g) * D;
        x0 = src[lane];
        x1 = src[lane + 64];
        if (w < 3) {
            const float* gam = w < 2 ? a.q_norm : a.k_norm;
            gm0 = gam[lane];
            gm1 = gam[lane + 64];
            cs = a.rope_cos[(size_t)pos * 64 + lane];
            sn = a.rope_sin[(size_t)pos * 64 + lane];
        }
    }
    float qpre = 0.f;
    if (MODE == ATTN_ATTEND && tid < 2 * D) qpre = row[(size_t)(2 * g) * D + tid];
    // APRE cached rows per 16-lane group are requested up front: 4 x 64 groups (1024 threads, one utterance) or
    // 8 x 16 groups (256 threads, a batch of 32) = the first 256 / 128 positions without a second memory round trip
    // (a batch-32 step at positions 65-113 took the dependent in-loop loads with APRE = 4: -0.8 % per frame with 8)
    h8 kpre[APRE], vpre[APRE];
    if (MODE != ATTN_PREP) {
#pragma unroll
        for (int i = 0; i < APRE; i++) {
            const int t = grp + i * ngrp;
            if (t < T) {
                kpre[i] = *(const h8*)(kbase + (size_t)t * D + l16 * 8);
                vpre[i] = *(const h8*)(vbase + (size_t)t * D + l16 * 8);
            }
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    Q3_PH(0);  // loads issued

    // ---- phase A: per-head RMSNorm + RoPE (rotate-half pairs i, i+64) ----
    if (MODE != ATTN_ATTEND) {
        if (w < 4) {
            if (w < 3) {
                float ss = wave_sum(x0 * x0 + x1 * x1);
                const float iv = 1.0f / sqrtf(ss / (float)D + a.eps);
                x0 = (x0 * iv) * gm0;
                x1 = (x1 * iv) * gm1;
                const float y0 = x0 * cs - x1 * sn;
                const float y1 = x1 * cs + x0 * sn;
                x0 = y0;
                x1 = y1;
            }
            if (w < 2) {
                if (MODE == ATTN_PREP) {
                    float* dst = row + (size_t)(2 * g + w) * D;
                    dst[lane] = x0;
                    dst[lane + 64] = x1;
                } else {
                    qs[w][lane] = x0;
                    qs[w][lane + 64] = x1;
                }
            } else {
                const half_t h0 = sat_half(x0), h1 = sat_half(x1);
                half_t* cd = (w == 2 ? a.kc : a.vc) + cbase + (size_t)pos * D;
                cd[lane] = h0;
                cd[lane + 64] = h1;
                float* nd = w == 2 ? knew : vnew;
                nd[lane] = (float)h0;
                nd[lane + 64] = (float)h1;
            }
        }
        if (MODE == ATTN_PREP) return;
    } else {
        if (tid < 2 * D) qs[tid / D][tid % D] = qpre;
    }
    __syncthreads();
    Q3_PH(1);  // phase A done (first global round trip + norm + rope), barrier passed

    // ---- phase B: online softmax per 16-lane group ----
    float q0[8], q1[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        q0[j] = qs[0][l16 * 8 + j] * a.scale;   // fold the 1/sqrt(D) into q once
        q1[j] = qs[1][l16 * 8 + j] * a.scale;
    }
    float m0 = -INFINITY, m1 = -INFINITY, l0 = 0.f, l1 = 0.f;
    float a0[8], a1[8];
#pragma unroll
    for (int j = 0; j < 8; j++) a0[j] = a1[j] = 0.f;

    // NOT restructured on purpose (e.g. the prefetched keys' scores hoisted out of their branches, so that their
    // reductions overlap): the compiler contracts `d += q * k` differently from call site to call site of this lambda --
    // in the ISA some sites compute the first two terms as v_fma_mix_f32 and the rest as v_pk_mul_f32 + v_add_f32, the
    // others all eight unfused, and which site does what differs per instantiation -- so moving the dot products changes
    // the low bits of some scores, and with them codec ids downstream.  Whoever restructures this pins the arithmetic
    // first (`#pragma clang fp contract(off)` in the dot product), as a change of its own that moves the bits knowingly.
    auto step = [&](const h8& kk, const h8& vv) {
        float d0 = 0.f, d1 = 0.f;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float kf = (float)kk[j];
            d0 += q0[j] * kf;
            d1 += q1[j] * kf;
        }
        // inside `if (t < T)`, which is uniform per 16-lane group: the whole exchange group is active (xlane_xor's contract)
        group_sum_down2<16>(d0, d1);
        const float n0 = fmaxf(m0, d0), n1 = fmaxf(m1, d1);
        const float c0 = __expf(m0 - n0), c1 = __expf(m1 - n1);   // exp(-inf) = 0 on the first row
        const float p0 = __expf(d0 - n0), p1 = __expf(d1 - n1);
        l0 = l0 * c0 + p0;
        l1 = l1 * c1 + p1;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float vf = (float)vv[j];
            a0[j] = a0[j] * c0 + p0 * vf;
            a1[j] = a1[j] * c1 + p1 * vf;
        }
        m0 = n0;
        m1 = n1;
    };
#pragma unroll
    for (int i = 0; i < APRE; i++) {
        const int t = grp + i * ngrp;
        if (t < T) step(kpre[i], vpre[i]);   // uniform per 16-lane group
    }
#pragma unroll 2
    for (int t = grp + APRE * ngrp; t < T; t += ngrp) {
        const h8 kk = *(const h8*)(kbase + (size_t)t * D + l16 * 8);
        const h8 vv = *(const h8*)(vbase + (size_t)t * D + l16 * 8);
        step(kk, vv);
    }
    if (MODE == ATTN_FUSED && grp == 0) {   // the token being appended, from LDS (fp16-rounded values)
        h8 kk, vv;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            kk[j] = (half_t)knew[l16 * 8 + j];
            vv[j] = (half_t)vnew[l16 * 8 + j];
        }
        step(kk, vv);
    }
    asm volatile("" ::"v"(a0[0]), "v"(l0));
    Q3_PH(2);  // cached rows + the new token processed
    // merge the 4 groups of a wave (lanes xor 16, 32), then the waves through LDS.
    // These two stages stay on __shfl_xor although every lane is active: 20 independent exchanges per stage overlap in
    // the LDS queue (two round trips on the critical path, not forty), and with them on permlane swaps the compiler
    // fuses the first terms of one more of step()'s dot products into v_fma_mix_f32 in the APRE = 8 instantiations
    // (16 instead of 12 in the ISA) -- other low bits in some scores, other codec ids downstream.  See the note at step().
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
        const float om0 = __shfl_xor(m0, o, 64), om1 = __shfl_xor(m1, o, 64);
        const float ol0 = __shfl_xor(l0, o, 64), ol1 = __shfl_xor(l1, o, 64);
        const float n0 = fmaxf(m0, om0), n1 = fmaxf(m1, om1);
        // a group that saw no row has m = -inf and l = 0: its scale is exp(-inf - n) = 0 unless n is -inf too
        const float c0 = (m0 == -INFINITY) ? 0.f : __expf(m0 - n0), d0 = (om0 == -INFINITY) ? 0.f : __expf(om0 - n0);
        const float c1 = (m1 == -INFINITY) ? 0.f : __expf(m1 - n1), d1 = (om1 == -INFINITY) ? 0.f : __expf(om1 - n1);
        l0 = l0 * c0 + ol0 * d0;
        l1 = l1 * c1 + ol1 * d1;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float oa0 = __shfl_xor(a0[j], o, 64), oa1 = __shfl_xor(a1[j], o, 64);
            a0[j] = a0[j] * c0 + oa0 * d0;
            a1[j] = a1[j] * c1 + oa1 * d1;
        }
        m0 = n0;
        m1 = n1;
    }
    if (lane < 16) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            pacc[(w * 2 + 0) * D + lane * 8 + j] = a0[j];
            pacc[(w * 2 + 1) * D + lane * 8 + j] = a1[j];
        }
        if (lane == 0) {
            pm[w * 2 + 0] = m0;
            pm[w * 2 + 1] = m1;
            pl[w * 2 + 0] = l0;
            pl[w * 2 + 1] = l1;
        }
    }
    __syncthreads();
    Q3_PH(3);  // groups merged, partials in LDS, barrier passed
    if (tid < 2 * D) {
        const int hh = tid / D, d = tid % D;
        float M = -INFINITY;
        for (int i = 0; i < nwv; i++) M = fmaxf(M, pm[i * 2 + hh]);
        float L = 0.f, o = 0.f;
        for (int i = 0; i < nwv; i++) {
            const float mi = pm[i * 2 + hh];
            const float c = (mi == -INFINITY) ? 0.f : __expf(mi - M);
            L += pl[i * 2 + hh] * c;
            o += pacc[(i * 2 + hh) * D + d] * c;
        }
        a.out[frag_idx(r, (2 * g + hh) * D + d, a.n_heads * D)] = sat_half(o / L);
    }
}

// ---------------------------------------------------------------------------
// attention over a short cache (code predictor: at most 15 cached positions + the token being appended):
// same phase A; then every 16-lane group scores at most two entries and parks them in LDS, and every
// (head, dim) thread finishes its own output -- max, exponentials, weighted sum over <= 32 entries with the
// V column it prefetched at kernel start.  No merge of partial softmaxes across groups and waves: two
// barriers, one short serial tail (the general kernel's merge + combine cost 1.9 of its 3.7 us here).
// ---------------------------------------------------------------------------
constexpr int ATTN_SHORT_MAX_T = 15;
static int g_attn_short = 1;
int set_attn_short(int on) { g_attn_short = on; return 0; }
// The leading arguments are what the first loads (the row's q / k / v, the norm weights, the RoPE row) need: 16 dwords that
// arrive in SGPRs at wave launch (-amdgpu-kernarg-preload-count=16, like linear_kernel); the rest of the struct is fetched
// in one batch under those loads' latency instead of in front of them.
__global__ void __launch_bounds__(256)
    attn_short_kernel(float* __restrict__ p_qkv, int p_ld, int p_row0, int p_n_heads, int p_n_kv,
                      const float* __restrict__ p_q_norm, const float* __restrict__ p_k_norm,
                      const float* __restrict__ p_rope_cos, const float* __restrict__ p_rope_sin, int p_pos_base,
                      int p_slot_base, AttnArgs a) {
    constexpr int D = 128, NE = ATTN_SHORT_MAX_T + 1;   // entries: <= 15 cached rows + the appended token
    a.qkv = p_qkv;
    a.ld = p_ld;
    a.row0 = p_row0;
    a.n_heads = p_n_heads;
    a.n_kv = p_n_kv;
    a.q_norm = p_q_norm;
    a.k_norm = p_k_norm;
    a.rope_cos = p_rope_cos;
    a.rope_sin = p_rope_sin;
    a.pos_base = p_pos_base;
    a.slot_base = p_slot_base;
    Q3_FETCH_ARGS("s"(a.eps), "s"(a.slot), "s"(a.slot_stride), "s"(a.kc), "s"(a.vc), "s"(a.n_ctx), "s"(a.out), "s"(a.scale));
    Q3_TL(33);
    const int r = a.row0 + blockIdx.x, g = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int slot = a.slot ? uniform_load(a.slot + r) : a.slot_base + r * a.slot_stride;
    const int T = a.pos_base;                       // cached rows = position of the appended token (row-uniform)
    __shared__ float qs[2][D];
    __shared__ float knew[D];
    __shared__ __attribute__((aligned(16))) half_t vs[NE][D];   // V rows of the entries (row T = the appended token)
    __shared__ __attribute__((aligned(16))) float sc[2][NE];
    float* row = a.qkv + (size_t)r * a.ld;
    const size_t cbase = ((size_t)slot * a.n_kv + g) * (size_t)a.n_ctx * D;
    const int l16 = tid & 15, grp = tid >> 4;       // 16 groups of 16 lanes: group e owns entry e
    const int hh = tid >> 7, d = tid & 127;         // the output this thread finishes
    // ---- every global load, issued up front: phase A operands, then this group's cached K and V row ----
    float x0 = 0.f, x1 = 0.f, gm0 = 1.f, gm1 = 1.f, cs = 1.f, sn = 0.f;
    {
        const float* src = w < 2 ? row + (size_t)(2 * g + w) * D
                         : w == 2 ? row + (size_t)(a.n_heads + g) * D
                                  : row + (size_t)(a.n_heads + a.n_kv + g) * D;
        x0 = src[lane];
        x1 = src[lane + 64];
        if (w < 3) {
            const float* gam = w < 2 ? a.q_norm : a.k_norm;
            gm0 = gam[lane];
            gm1 = gam[lane + 64];
            cs = a.rope_cos[(size_t)T * 64 + lane];
            sn = a.rope_sin[(size_t)T * 64 + lane];
        }
    }
    h8 kpre, vpre;
    if (grp < T) {
        kpre = *(const h8*)(a.kc + cbase + (size_t)grp * D + l16 * 8);
        vpre = *(const h8*)(a.vc + cbase + (size_t)grp * D + l16 * 8);
    }
    __builtin_amdgcn_sched_barrier(0);
    Q3_PH(0);
    // ---- phase A: per-head RMSNorm + RoPE, K/V appended (identical arithmetic to attn_kernel) ----
    if (w < 3) {
        float ss = wave_sum(x0 * x0 + x1 * x1);
        const float iv = 1.0f / sqrtf(ss / (float)D + a.eps);
        x0 = (x0 * iv) * gm0;
        x1 = (x1 * iv) * gm1;
        const float y0 = x0 * cs - x1 * sn;
        const float y1 = x1 * cs + x0 * sn;
        x0 = y0;
        x1 = y1;
    }
    if (w < 2) {
        qs[w][lane] = x0;
        qs[w][lane + 64] = x1;
    } else {
        const half_t h0 = sat_half(x0), h1 = sat_half(x1);
        half_t* cd = (w == 2 ? a.kc : a.vc) + cbase + (size_t)T * D;
        cd[lane] = h0;
        cd[lane + 64] = h1;
        if (w == 2) {
            knew[lane] = (float)h0;
            knew[lane + 64] = (float)h1;
        } else {
            vs[T][lane] = h0;
            vs[T][lane + 64] = h1;
        }
    }
    if (grp < T) *(h8*)(&vs[grp][l16 * 8]) = vpre;   // cached V rows parked for the last phase
    __syncthreads();
    Q3_PH(1);
    // ---- scores: entry e < T from the cache, entry T = the appended token (fp16-rounded, from LDS) ----
    if (grp <= T) {   // uniform per 16-lane group
        float d0 = 0.f, d1 = 0.f;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float kf = grp < T ? (float)kpre[j] : knew[l16 * 8 + j];
            d0 += (qs[0][l16 * 8 + j] * a.scale) * kf;
            d1 += (qs[1][l16 * 8 + j] * a.scale) * kf;
        }
        group_sum_down2<16>(d0, d1);
        if (l16 == 0) {
            sc[0][grp] = d0;
            sc[1][grp] = d1;
        }
    }
    __syncthreads();
    Q3_PH(2);
    // ---- every (head, dim) thread: softmax over the T+1 scores, weighted sum of its V column ----
    float sv[NE];
#pragma unroll
    for (int e4 = 0; e4 < NE; e4 += 4) {     // 4 broadcast reads of 16 B
        const float4 t4 = *(const float4*)(&sc[hh][e4]);
        sv[e4] = t4.x;
        sv[e4 + 1] = t4.y;
        sv[e4 + 2] = t4.z;
        sv[e4 + 3] = t4.w;
    }
    float m = -INFINITY;
#pragma unroll
    for (int e = 0; e < NE; e++) m = fmaxf(m, e <= T ? sv[e] : -INFINITY);
    float L = 0.f, o = 0.f;
#pragma unroll
    for (int e = 0; e < NE; e++) {
        const float p = e <= T ? __expf(sv[e] - m) : 0.f;       // (rows beyond T hold stale LDS: masked, never NaN-multiplied)
        const float vf = e <= T ? (float)vs[e][d] : 0.f;
        L += p;
        o += p * vf;
    }
    Q3_PH(3);
    a.out[frag_idx(r, (2 * g + hh) * D + d, a.n_heads * D)] = sat_half(o / L);
}

// ---------------------------------------------------------------------------
// attn_tile_mfma_kernel -- the ATTEND step of a prefill for a tile of up to 16 consecutive positions of one utterance
// and one kv head (2 q heads = 32 query rows); K/V of the tile's own positions are already in the cache (ATTN_PREP).
// The generic kernel spends one workgroup per (row, kv head): 7 768 workgroups of a microsecond each for the
// benchmark's 971-row prefill, 30 us per layer.  Here both products run on the MFMA (v_mfma_f32_16x16x32_f16):
// S = Q.K^T with K rows straight from the cache image (the B operand wants 8 consecutive head dims of one key: a K
// row), O = P.V with V rows staged as they are and read through the hardware transposing LDS read
// (ds_read_b64_tr_b16: a 16-lane group reads a 4 x 16 block and every lane receives one COLUMN of it -- the B operand
// wants 8 consecutive keys of one head dim).  The contract keeps q and the softmax in f32: q and P are carried as two fp16 terms (hi,
// lo = fp16((x - hi) * 2048)), two MFMAs per product, recombined in f32 -- 22 mantissa bits, the fp16 K / V values
// exact.  Wave w owns keys 16w..16w+15 of a 64-key chunk for S and head dims 32w..32w+31 for O; row maxima and sums
// meet through LDS; the O accumulators share S's row layout, so the online-softmax rescale needs no data movement.
// Every global load of a chunk (and, for the first, the queries) is issued before anything waits.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) attn_tile_mfma_kernel(AttnArgs a) {
    constexpr int D = 128, QP = 136, VP = 72, CH = 64;
    constexpr float LO = 2048.0f, ILO = 1.0f / 2048.0f;
    Q3_TL(35);
    const int g = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = lane & 15, q4 = lane >> 4;
    int row0, nrows, slot, pos0;
    if (a.tiles) {
        const int4 t = *(const int4*)(a.tiles + 4 * blockIdx.x);
        row0 = t.x; nrows = t.y; slot = t.z; pos0 = t.w;
    } else {   // one run of consecutive positions of one slot
        row0 = a.row0 + blockIdx.x * 16;
        nrows = a.R - blockIdx.x * 16 < 16 ? a.R - blockIdx.x * 16 : 16;
        slot = a.slot_base;
        pos0 = a.pos_base + blockIdx.x * 16;
    }
    extern __shared__ __attribute__((aligned(16))) char smem[];
    half_t* qh = (half_t*)smem;                 // [32][QP]   query rows: head * 16 + position, pre-scaled, hi term
    half_t* ql = qh + 32 * QP;                  // [32][QP]   lo term
    half_t* ks = ql + 32 * QP;                  // [CH][QP]   K rows of the chunk
    half_t* vs = ks + CH * QP;                  // [CH][QP]   V rows of the chunk
    half_t* ph = vs + CH * QP;                  // [32][VP]   P hi
    half_t* pl = ph + 32 * VP;                  // [32][VP]   P lo
    float* red = (float*)(pl + 32 * VP);        // [4][32] per-wave row maxima, then [4][32] row sums
    float* red2 = red + 4 * 32;
    const size_t cbase = ((size_t)slot * a.n_kv + g) * (size_t)a.n_ctx * D;
    const int T = pos0 + nrows;
    // K and V chunks: thread -> 4 pieces of 16 B each, rows idx / 16 (coalesced 256-B rows), zeros beyond T
    h8 kreg[4], vreg[4];
    auto load_chunk = [&](int c0) {
#pragma unroll
        for (int it = 0; it < 4; it++) {
            const int idx = tid + it * 256, kr = idx >> 4, d8 = (idx & 15) * 8;
            kreg[it] = vreg[it] = (h8){0, 0, 0, 0, 0, 0, 0, 0};
            if (c0 + kr < T) {
                kreg[it] = *(const h8*)(a.kc + cbase + (size_t)(c0 + kr) * D + d8);
                vreg[it] = *(const h8*)(a.vc + cbase + (size_t)(c0 + kr) * D + d8);
            }
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int it = 0; it < 4; it++) {
            const int idx = tid + it * 256, kr = idx >> 4, d8 = (idx & 15) * 8;
            *(h8*)(ks + kr * QP + d8) = kreg[it];
            *(h8*)(vs + kr * QP + d8) = vreg[it];
        }
    };
    load_chunk(0);          // in flight together with the query rows
    for (int idx = tid; idx < 32 * (D / 8); idx += 256) {
        const int qr = idx / (D / 8), d8 = (idx - qr * (D / 8)) * 8, i = qr & 15, hh = qr >> 4;
        h8 hi = {0, 0, 0, 0, 0, 0, 0, 0}, lo = hi;
        if (i < nrows) {
            const float* src = a.qkv + (size_t)(row0 + i) * a.ld + (size_t)(2 * g + hh) * D + d8;
            const float4 v0 = *(const float4*)src, v1 = *(const float4*)(src + 4);
            const float e[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const float x = e[j] * a.scale;
                hi[j] = sat_half(x);
                lo[j] = (half_t)((x - (float)hi[j]) * LO);
            }
        }
        *(h8*)(qh + qr * QP + d8) = hi;
        *(h8*)(ql + qr * QP + d8) = lo;
    }
    // rows this lane sees in every accumulator fragment: head qb, position 4 * q4 + r
    float mrow[2][4], lrow[2][4];
    f4 oh[2][2], ol[2][2];
#pragma unroll
    for (int qb = 0; qb < 2; qb++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            mrow[qb][r] = -INFINITY;
            lrow[qb][r] = 0.f;
        }
#pragma unroll
    for (int qb = 0; qb < 2; qb++)
#pragma unroll
        for (int j = 0; j < 2; j++) oh[qb][j] = ol[qb][j] = (f4){0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < T; c0 += CH) {
        __syncthreads();                                    // previous chunk consumed
        store_chunk();                                      // (keys beyond T are zeros; their P is exactly 0 anyway)
        if (c0 + CH < T) load_chunk(c0 + CH);               // the next chunk travels under this chunk's products
        __syncthreads();
        // ---- S = Q.K^T for keys 16w .. 16w+15 of the chunk ----
        f4 sh[2], sl[2];
        sh[0] = sh[1] = sl[0] = sl[1] = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < 4; kb++) {
            const h8 bk = *(const h8*)(ks + (16 * w + c) * QP + kb * 32 + q4 * 8);
#pragma unroll
            for (int qb = 0; qb < 2; qb++) {
                const h8 ahi = *(const h8*)(qh + (16 * qb + c) * QP + kb * 32 + q4 * 8);
                const h8 alo = *(const h8*)(ql + (16 * qb + c) * QP + kb * 32 + q4 * 8);
                sh[qb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi, bk, sh[qb], 0, 0, 0);
                sl[qb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(alo, bk, sl[qb], 0, 0, 0);
            }
        }
        const int key = c0 + 16 * w + c;
        float sc[2][4], mx[2][4];
#pragma unroll
        for (int qb = 0; qb < 2; qb++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int i = 4 * q4 + r;
                float v = sh[qb][r] + sl[qb][r] * ILO;
                if (!(i < nrows && key <= pos0 + i)) v = -INFINITY;          // causal mask, rows beyond the tile
                sc[qb][r] = v;
                const float x = group_max_up<16>(v);
                mx[qb][r] = x;
                if (c == 0) red[w * 32 + 16 * qb + i] = x;
            }
        __syncthreads();
        float corr[2][4];
#pragma unroll
        for (int qb = 0; qb < 2; qb++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int qr = 16 * qb + 4 * q4 + r;
                const float cm = fmaxf(fmaxf(red[qr], red[32 + qr]), fmaxf(red[64 + qr], red[96 + qr]));
                const float mo = mrow[qb][r], mn = fmaxf(mo, cm);
                corr[qb][r] = (mo == -INFINITY) ? 0.f : __expf(mo - mn);
                const float p = (sc[qb][r] == -INFINITY) ? 0.f : __expf(sc[qb][r] - mn);
                const half_t hi = (half_t)p;
                ph[qr * VP + 16 * w + c] = hi;
                pl[qr * VP + 16 * w + c] = (half_t)((p - (float)hi) * LO);
                const float ssum = group_sum_up<16>(p);
                if (c == 0) red2[w * 32 + qr] = ssum;
                mrow[qb][r] = mn;
            }
        __syncthreads();
#pragma unroll
        for (int qb = 0; qb < 2; qb++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int qr = 16 * qb + 4 * q4 + r;
                lrow[qb][r] = lrow[qb][r] * corr[qb][r] + ((red2[qr] + red2[32 + qr]) + (red2[64 + qr] + red2[96 + qr]));
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    oh[qb][j][r] *= corr[qb][r];
                    ol[qb][j][r] *= corr[qb][r];
                }
            }
        // ---- O += P.V for head dims 32w .. 32w+31 ----
#pragma unroll
        for (int kst = 0; kst < 2; kst++) {
#pragma unroll
            for (int j = 0; j < 2; j++) {
                // B[k = 8 * q4 + e][column c] = V[key kst * 32 + 8 * q4 + e][head dim 32w + 16j + c]: lane 4q + p of a
                // 16-lane group addresses row q, columns 4p .. 4p+3 of a 4 x 16 block and receives column (lane & 15)
                typedef __fp16 hv4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
                const half_t* vb = vs + (kst * 32 + 8 * q4 + (c >> 2)) * QP + 32 * w + 16 * j + 4 * (c & 3);
                const hv4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) hv4*)vb);
                const hv4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) hv4*)(vb + 4 * QP));
                h8 bv;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    bv[e] = (half_t)t0[e];
                    bv[4 + e] = (half_t)t1[e];
                }
#pragma unroll
                for (int qb = 0; qb < 2; qb++) {
                    const h8 ahi = *(const h8*)(ph + (16 * qb + c) * VP + kst * 32 + q4 * 8);
                    const h8 alo = *(const h8*)(pl + (16 * qb + c) * VP + kst * 32 + q4 * 8);
                    oh[qb][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi, bv, oh[qb][j], 0, 0, 0);
                    ol[qb][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(alo, bv, ol[qb][j], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int qb = 0; qb < 2; qb++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int i = 4 * q4 + r;
            if (i < nrows) {
                const float inv = 1.0f / lrow[qb][r];
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const float o = (oh[qb][j][r] + ol[qb][j][r] * ILO) * inv;
                    a.out[frag_idx(row0 + i, (2 * g + qb) * D + 32 * w + 16 * j + c, a.n_heads * D)] = sat_half(o);
                }
            }
        }
}

int launch_attn(hipStream_t s, const AttnArgs& a, int mode) {
    if (a.R <= 0) return 0;
    if (a.n_heads != 2 * a.n_kv) {
        Q3_LOG("attn: only GQA group 2 (16q/8kv) is built, got %d/%d", a.n_heads, a.n_kv);
        return -1;
    }
    // every row at the same short position, known on the host (the code predictor's passes): the short-cache kernel
    if (g_attn_short && mode == ATTN_FUSED && !a.pos && a.pos_stride == 0 && a.pos_base >= 0 &&
        a.pos_base <= ATTN_SHORT_MAX_T && a.pos_base < a.n_ctx) {
        AttnArgs a3 = a;
        a3.tl_node = tl_next_node();
        hipLaunchKernelGGL(attn_short_kernel, dim3(a.R, a.n_kv), dim3(256), 0, s, a3.qkv, a3.ld, a3.row0, a3.n_heads, a3.n_kv,
                           a3.q_norm, a3.k_norm, a3.rope_cos, a3.rope_sin, a3.pos_base, a3.slot_base, a3);
        Q3_HIP(hipGetLastError(), -1);
        return 0;
    }
    // prefill: runs of consecutive positions of one utterance -> 16-position tiles
    // prefill: runs of consecutive positions of one utterance -> 16-position tiles on the MFMA
    if (mode == ATTN_ATTEND && a.n_tiles > 0) {
        constexpr size_t lds = (size_t)(2 * 32 * 136 + 2 * 64 * 136 + 2 * 32 * 72) * 2 + 8 * 32 * 4;
        static bool attr = false;
        if (!attr) {
            Q3_HIP(hipFuncSetAttribute((const void*)attn_tile_mfma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), -1);
            attr = true;
        }
        AttnArgs a5 = a;
        a5.tl_node = tl_next_node();
        hipLaunchKernelGGL(attn_tile_mfma_kernel, dim3(a.n_tiles, a.n_kv), dim3(256), lds, s, a5);
        Q3_HIP(hipGetLastError(), -1);
        return 0;
    }
    // keep the launch small: ~64K threads fill in ~2 us, every further 64K cost ~1 us of ramp
    int threads = a.threads;
    const int fit = 65536 / (a.R * a.n_kv);     // (round 3: 512 threads per workgroup at batch 32 -- 131 072 in all -- changed nothing: 2.41 ms per frame either way)
    if (threads > fit) threads = fit / 64 * 64;
    if (threads < 256) threads = 256;
    if (threads > 1024) threads = 1024;
    const size_t lds = ((size_t)(threads / 64) * (4 + 2 * 128)) * sizeof(float);
    AttnArgs a2 = a;
    a2.tl_node = tl_next_node();
    dim3 grid(a.R, a.n_kv);
#define Q3_ATTN(MODE_)                                                                                   \
    {                                                                                                    \
        if (threads <= 256)                                                                              \
            hipLaunchKernelGGL((attn_kernel<MODE_, 8>), grid, dim3(256), mode == ATTN_PREP ? 0 : lds, s, a2); \
        else                                                                                             \
            hipLaunchKernelGGL((attn_kernel<MODE_, 4>), grid, dim3(mode == ATTN_PREP ? 256 : threads),   \
                               mode == ATTN_PREP ? 0 : lds, s, a2);                                      \
    }
    if (mode == ATTN_FUSED) Q3_ATTN(ATTN_FUSED)
    else if (mode == ATTN_PREP) Q3_ATTN(ATTN_PREP)
    else Q3_ATTN(ATTN_ATTEND)
#undef Q3_ATTN
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

}  // namespace q3
