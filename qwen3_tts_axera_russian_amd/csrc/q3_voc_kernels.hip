// q3_voc_kernels.hip -- the vocoder's kernels for gfx950, each with the launcher that picks its variant and grid
// (declared in q3_voc_ops.h).  The program that strings them together is q3_voc.hip, the streaming walks q3_voc_stream.hip.
//
//   rvq_kernel     16 codebook gathers per frame, summed per quantiser half, two 256->512 projections
//   conv_kernel    causal Conv1d / polyphase ConvTranspose1d as an implicit GEMM on the exact-fp32 MFMA
//                  (v_mfma_f32_32x32x2_f32): one input tile [8 ch][128+halo] is staged once in LDS (the
//                  line buffer) and read at every dilated tap offset; Snake is applied while staging,
//                  bias / residual add / clamp in the epilogue.
#include "../../include/qwen3tts_voc.h"
#include "q3_common.h"
#include "q3_voc_ops.h"

#include <algorithm>
#include <cmath>

namespace q3 {

typedef float f16v __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float elu1(float x) { return x > 0.f ? x : expm1f(x); }   // ELU, alpha = 1

// test hook (voc_debug_last_variant at the end of this file; host side only): the instantiation the last conv (or full-chunk
// attention) launch of this thread took (a few plain stores per launch; named on request)
enum { VV_NONE, VV_CONV, VV_OUT1, VV_RESUNIT, VV_SNAKE_SPLIT, VV_SPLIT, VV_ATTN_TILE, VV_ATTN };
static thread_local struct {
    int kind = VV_NONE, p[5] = {0, 0, 0, 0, 0};
    bool after_pass = false;   // split conv: its planes came from snake_split_kernel right before it
} voc_variant;
static inline void voc_note_variant(int kind, int a = 0, int b = 0, int c = 0, int d = 0, int e = 0) {
    voc_variant.after_pass = kind == VV_SPLIT && voc_variant.kind == VV_SNAKE_SPLIT;
    voc_variant.kind = kind;
    voc_variant.p[0] = a, voc_variant.p[1] = b, voc_variant.p[2] = c, voc_variant.p[3] = d, voc_variant.p[4] = e;
}
constexpr int VKC = 8;     // input channels per LDS stage
constexpr int VTN = 128;   // output columns per workgroup (4 waves x 32)
// LDS row pitches of the staged operands.  An MFMA operand read is 64 lanes x 4 B: lanes 0-31 walk 32 consecutive floats of
// row ci, lanes 32-63 of row ci + 1; the two halves hit disjoint banks when the row pitch is 32 mod 64 floats.
// (round 3, per-op profile at 32 chunks: the input tile's pitch padded that way removes every bank conflict of the 7-tap and fused
// kernels -- SQ_LDS_BANK_CONFLICT 0 -- and takes 1.5 % off the decode, 92.5 -> 91.1 ms; padding the weight rows too costs LDS
// and gains nothing)
#ifndef Q3_VOC_XPAD
#define Q3_VOC_XPAD 1
#endif
#ifndef Q3_VOC_WPAD
#define Q3_VOC_WPAD 0
#endif
__host__ __device__ constexpr int voc_wpitch(int TM) { return Q3_VOC_WPAD ? (TM % 64 == 0 ? TM + 32 : (TM % 64 == 32 ? TM : TM + 4)) : TM + 4; }
__host__ __device__ inline int voc_xpitch(int XW) { return Q3_VOC_XPAD ? ((XW + 31) / 64) * 64 + 32 : XW; }

// conv_kernel<MT, KT, KC>: MT 32-row MFMA tiles per wave, KT taps, KC input channels per LDS stage.
// Staging goes global -> LDS directly; ~4 workgroups per CU hide its latency (a register-staged software
// pipeline was tried: 199-256 VGPRs, one workgroup per SIMD, 1.6x slower at 32 chunks).
// ACT: what is applied to the input while it is staged -- 0 nothing, 1 Snake, 2 exact GELU, 3 decided at run time (a.alpha /
// a.gelu), 4 ELU (the speech-tokenizer encoder, a.elu; never chosen at run time, so the other variants compile as before).  Compiled in for the one-tap convs (round 3, per-op profile at 32 chunks: the Snake 1 x 1 convs that close the 768- /
// 384-channel residual units 0.82 -> 0.75 and 1.27 -> 1.11 ms); for two and more taps the run-time form is the faster one
// (7-tap 126 vs 124 TFLOP/s, transposed convs 105 vs 99: the specialised kernels are scheduled worse), so those keep it.
template <int MT, int KT, int KC, bool CT = false, int ACT = 3>   // CT: transposed conv (stride > 1, no residual), stores go through an LDS slab
__global__ void __launch_bounds__(256, (KC >= 32 && MT >= 3) ? 2 : (MT >= 4 ? 3 : (MT == 3 ? 3 : 4))) conv_kernel(ConvArgs a) {
    constexpr int TM = 32 * MT, TMP = voc_wpitch(TM), Q = KC / 4;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int halo = (KT - 1) * a.dil;
    // staged columns: l0-HA .. l0+127, HA = the halo rounded up to 4 columns, so that the tile starts on a 16-byte boundary of
    // its row and is fetched as float4 groups (round 3: as 4-byte loads -- six per thread and stage, each with its own bounds
    // logic and LDS store -- the input tile cost as much as the five times larger weight tile; timing with either staging
    // compiled out)
    const int HA = (halo + 3) & ~3;
    const int XW = VTN + HA;
    const int XP = voc_xpitch(XW);     // their row pitch in LDS
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Ws = lds;                   // [KT][KC][TMP]
    float* Xs = lds + KT * KC * TMP;   // [KC][XP]
    // persistent over output tiles (the grid may be capped, see voc_set_max_workgroups)
    for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const int lx = tile % a.tiles_l, my = (tile / a.tiles_l) % a.tiles_m, b = tile / (a.tiles_l * a.tiles_m);
        const int l0 = lx * VTN, m0 = my * TM;
        const float* xb = a.x + (size_t)b * a.Cin * a.ldx;
        const int Lcols = a.flat_B > 0 ? a.flat_B * a.ldx : a.Lc;   // columns of the tiled axis (flattened: pads included)
        f16v acc[MT];
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int i = 0; i < 16; i++) acc[mt][i] = 0.f;
        // Weights of all taps for KC channels.  Packed layout [ci/8][k][ci%8][Mp] (rows contiguous): a tile row is
        // TM contiguous floats, copied with 16-B loads / ds_write_b128, no transposition
        constexpr int WN = KT * KC * (TM / 4), WIT = (WN + 255) / 256;
        constexpr int LPC = 256 / KC;
        constexpr int XJ1 = (VTN / 4 + LPC - 1) / LPC;   // one-tap path: float4 groups of the input tile per thread
        const int xci = tid / LPC, xl = tid - xci * LPC;
        float4 wv[WIT];
        float4 xv1[KT == 1 ? XJ1 : 1];
        float al = 0.f, ib = 0.f;
        // Staging issues EVERY global load of a stage before the first use (fixed trip counts, clamped addresses,
        // predicated results): a load inside an `if` gets its own s_waitcnt in that branch, which made the stage a
        // chain of dependent round trips (one per 256 elements) instead of one.
        auto load_w = [&](int ci0) {
#pragma unroll
            for (int i = 0; i < WIT; i++) {
                const int idx = tid + i * 256, ic = idx < WN ? idx : 0;
                const int m4 = ic % (TM / 4), ci = (ic / (TM / 4)) % KC, k = ic / ((TM / 4) * KC);
                const int m = m0 + m4 * 4, mc = m < a.Mp ? m : 0, cg = ci0 + ci;
                wv[i] = *(const float4*)(a.wk + (unsigned)((((cg >> 3) * KT + k) * 8 + (cg & 7)) * a.Mp + mc));
                if (m >= a.Mp) wv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            // the input line buffer (causal: columns left of 0 are zero; Snake(0) = 0 so padding commutes).  A thread
            // stays on ONE channel of the stage (LPC lanes per channel), so its Snake parameters are two registers
            if (ACT == 1 || (ACT == 3 && a.alpha)) { al = a.alpha[ci0 + xci]; ib = a.inv_beta[ci0 + xci]; }
        };
        auto load_x1 = [&](int ci0) {   // one tap: no halo, the tile's 128 columns start 16-byte aligned
#pragma unroll
            for (int j = 0; j < (KT == 1 ? XJ1 : 1); j++) {
                const int c4 = (xl + j * LPC) * 4, c4c = c4 < VTN ? c4 : 0;
                const int gl = l0 + c4c, glc = gl < Lcols ? gl : 0;
                const int bb = a.flat_B > 0 ? glc / a.ldx : 0, l = glc - bb * a.ldx;   // (4 | ldx: a group stays in its chunk)
                xv1[j] = *(const float4*)(xb + (unsigned)((bb * a.Cin + ci0 + xci) * a.ldx + l));
            }
        };
        // One tap: the stage is short (KC / 2 MFMAs per row tile), so the NEXT stage's operands are requested into
        // registers before this stage's MFMAs and land under them (2 + 2 float4 per thread at 16 channels); with more
        // taps the prefetch registers cost a workgroup per CU (tried: 1.6x slower).
        // (32-channel stages keep the plain form: 16 + 16 more live registers put the 128-row tile 99 registers over)
        const bool al1 = KT == 1;                           // one tap: 16-byte staging (rows are 16-byte aligned: 4 | ldx)
        const bool pre1 = al1 && KC <= 16;                  // ... with the next stage prefetched
        if (pre1) {
            load_w(0);
            load_x1(0);
        }
        for (int ci0 = 0; ci0 < a.Cin; ci0 += KC) {
            __syncthreads();  // previous stage (or tile) fully consumed
            if (!pre1) {
                load_w(ci0);
                if (al1) load_x1(ci0);
            }
            auto store_w = [&]() {
#pragma unroll
                for (int i = 0; i < WIT; i++) {
                    const int idx = tid + i * 256;
                    if (idx < WN) {
                        const int m4 = idx % (TM / 4), ci = (idx / (TM / 4)) % KC, k = idx / ((TM / 4) * KC);
                        *(float4*)(Ws + (k * KC + ci) * TMP + m4 * 4) = wv[i];
                    }
                }
            };
            if (al1) {
                // operands of this stage are in registers (requested a stage ago when prefetching) -> ds_write_b128
                store_w();
#pragma unroll
                for (int j = 0; j < (KT == 1 ? XJ1 : 1); j++) {
                    const int c4 = (xl + j * LPC) * 4;
                    if (c4 < VTN) {
                        float4 v = xv1[j];
                        if (ACT == 1 || (ACT == 3 && a.alpha)) {
                            float sn;
                            sn = __sinf(al * v.x); v.x = v.x + ib * (sn * sn);
                            sn = __sinf(al * v.y); v.y = v.y + ib * (sn * sn);
                            sn = __sinf(al * v.z); v.z = v.z + ib * (sn * sn);
                            sn = __sinf(al * v.w); v.w = v.w + ib * (sn * sn);
                        }
                        if (ACT == 2 || (ACT == 3 && a.gelu)) {
                            v.x = gelu_erf(v.x); v.y = gelu_erf(v.y); v.z = gelu_erf(v.z); v.w = gelu_erf(v.w);
                        }
                        if (ACT == 4) {
                            v.x = elu1(v.x); v.y = elu1(v.y); v.z = elu1(v.z); v.w = elu1(v.w);
                        }
                        if (l0 + c4 >= Lcols) v = make_float4(0.f, 0.f, 0.f, 0.f);
                        *(float4*)(Xs + xci * XP + c4) = v;
                    }
                }
            } else {
                // float4 groups of the tile: (VTN + HA) / 4 per channel, dealt to the LPC lanes of the channel (dilation <= 9: launcher)
                constexpr int XG = (VTN + (((KT - 1) * 9 + 3) & ~3)) / 4, XJ = (XG + LPC - 1) / LPC;
                float4 xv[XJ];
#pragma unroll
                for (int j = 0; j < XJ; j++) {
                    const int c4 = (xl + j * LPC) * 4;
                    // a group is wholly left of column 0 or not at all (l0 - HA is a multiple of 4); its row is 16-byte aligned
                    // (4 | ldx) and padded to the pitch, so a group that straddles Lin reads allocated columns
                    const int l = l0 - HA + c4, lc = (c4 < XW && l >= 0 && l < a.Lin) ? l : 0;
                    xv[j] = *(const float4*)(xb + (unsigned)((ci0 + xci) * a.ldx + lc));
                }
                store_w();
#pragma unroll
                for (int j = 0; j < XJ; j++) {
                    const int c4 = (xl + j * LPC) * 4;
                    if (c4 < XW) {
                        const int l = l0 - HA + c4;
                        float4 v = xv[j];
                        if (ACT == 1 || (ACT == 3 && a.alpha)) {
                            float sn;
                            sn = __sinf(al * v.x); v.x = v.x + ib * (sn * sn);
                            sn = __sinf(al * v.y); v.y = v.y + ib * (sn * sn);
                            sn = __sinf(al * v.z); v.z = v.z + ib * (sn * sn);
                            sn = __sinf(al * v.w); v.w = v.w + ib * (sn * sn);
                        }
                        if (ACT == 2 || (ACT == 3 && a.gelu)) {
                            v.x = gelu_erf(v.x); v.y = gelu_erf(v.y); v.z = gelu_erf(v.z); v.w = gelu_erf(v.w);
                        }
                        if (ACT == 4) {
                            v.x = elu1(v.x); v.y = elu1(v.y); v.z = elu1(v.z); v.w = elu1(v.w);
                        }
                        if (l < 0) v = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (l >= a.Lin) v.x = 0.f;
                        if (l + 1 >= a.Lin) v.y = 0.f;
                        if (l + 2 >= a.Lin) v.z = 0.f;
                        if (l + 3 >= a.Lin) v.w = 0.f;
                        *(float4*)(Xs + xci * XP + c4) = v;
                    }
                }
            }
            __syncthreads();
            if (pre1 && ci0 + KC < a.Cin) {   // the next stage's operands: in flight under this stage's MFMAs
                load_w(ci0 + KC);
                load_x1(ci0 + KC);
            }
            // (round 3 probes of this loop, all measured per op at 32 chunks: the compiler's own schedule -- two A reads, wait, two
            // MFMAs, twice per step -- beats "all reads, one wait, four MFMAs" by 5 % (forced with sched_barrier: 91.1 -> 96.4 ms
            // per decode), and a hand-made software pipeline that issues half-step t + 1's LDS reads before half-step t's MFMAs
            // is worth 1 % at 17 spilled registers; 3 workgroups per CU run as fast as 4; co-resident workgroups started a quarter stage
            // apart: no change.  With the staging of all but the first stage compiled out (wrong results, timing only) the 7-tap
            // convs run at 139-140 TFLOP/s = 89 % and the transposed ones at 130-134 = 84 %, with or without the two barriers:
            // the loop itself holds 11-16 % of the peak back, the staging WORK (global loads, Snake, LDS writes -- not the barriers)
            // another 10 % of the 7-tap and 20 % of the transposed convs.)
#pragma unroll 1
            for (int k = 0; k < KT; k++) {
                const int off = HA - (KT - 1 - k) * a.dil + w * 32 + (lane & 31);
#pragma unroll
                for (int kk = 0; kk < KC; kk += 2) {
                    const int ci = kk + (lane >> 5);
                    const float bv = Xs[ci * XP + off];
#pragma unroll
                    for (int mt = 0; mt < MT; mt++) {
                        const float av = Ws[(k * KC + ci) * TMP + mt * 32 + (lane & 31)];
                        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[mt], 0, 0, 0);
                    }
                }
            }
        }
        // epilogue.  D layout: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
        const int gl = l0 + w * 32 + (lane & 31);
        const int be = a.flat_B > 0 ? gl / a.ldx : b;
        const int l = a.flat_B > 0 ? gl - be * a.ldx : gl;
        if constexpr (CT) {
            // transposed conv: row m = co * stride + p lands at y[co][l * stride + p] -- stored straight from the D
            // layout that is one 4-byte store per lane at a stride of `stride` floats (32-byte sectors filled a few
            // bytes at a time).  Each 32-row tile goes through LDS instead and leaves as runs of 128 * stride
            // consecutive floats per output channel.
            constexpr int TP = VTN + 1;
            float* T = lds;   // [32][TP] (the launcher sizes the LDS request for it)
            const int s = a.stride;
#pragma unroll   // (static register indices: a rolled loop would put the accumulators in scratch)
            for (int mt = 0; mt < MT; mt++) {
                __syncthreads();   // the last stage's operands (or the previous slab) are consumed
#pragma unroll
                for (int r = 0; r < 16; r++)
                    T[((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * TP + w * 32 + (lane & 31)] = acc[mt][r];
                __syncthreads();
                const int m_lo = m0 + mt * 32, m_hi = (m_lo + 32 < a.M) ? m_lo + 32 : a.M;
                if (m_lo < m_hi) {
                    const int ncol = (a.Lc - l0 < VTN) ? a.Lc - l0 : VTN;   // live columns of this tile
                    for (int co = m_lo / s; co * s < m_hi; co++) {
                        const float bv = a.bias ? a.bias[co] : 0.f;
                        float* yrow = a.y + (size_t)b * a.Cout * a.ldy + (unsigned)(co * a.ldy);
                        for (int j = tid; j < ncol * s; j += 256) {
                            const int lc = j / s, ph = j - lc * s, m = co * s + ph;
                            const int jo = l0 * s + j - a.lt;                     // output column after the left trim
                            if (m >= m_lo && m < m_hi && jo >= 0 && jo < a.Lout) {
                                float v = T[(m - m_lo) * TP + lc] + bv;
                                if (a.clamp) v = fminf(fmaxf(v, -1.f), 1.f);
                                __builtin_nontemporal_store(v, &yrow[jo]);
                            }
                        }
                    }
                }
            }
        } else if (gl < Lcols) {
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int m = m0 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    if (m < a.M) {
                        const int co = a.stride == 1 ? m : m / a.stride;
                        const int p = a.stride == 1 ? 0 : m % a.stride;
                        const int jo = l * a.stride + p - a.lt;                    // (stride 1: lt = 0, every column is kept)
                        if (a.stride != 1 && (jo < 0 || jo >= a.Lout)) continue;
                        const unsigned idx = (unsigned)((be * a.Cout + co) * a.ldy + jo);   // (launcher: < 2^31)
                        float v = acc[mt][r];
                        if (a.bias) v += a.bias[co];
                        if (a.res) v += a.res[idx];
                        if (a.clamp) v = fminf(fmaxf(v, -1.f), 1.f);
                        // streaming store: activations are far larger than L2 and are read next by another launch; a
                        // line left dirty in L2 is written back at the NEXT kernel boundary of any queue -- the frame
                        // loop's, 553 times per frame, when the vocoder runs beside it
                        __builtin_nontemporal_store(v, &a.y[idx]);
                    }
                }
        }
    }  // tile loop
}

template <int MT, int KT, int KC, bool CT = false, int ACT = -1>
static int launch_conv_t(hipStream_t s, const ConvArgs& a, int B, const VocSettings& cfg) {
    if constexpr (!CT && KT <= 2) {
        if (a.stride > 1 && a.res == nullptr) return launch_conv_t<MT, KT, KC, true, ACT>(s, a, B, cfg);
    }
    if constexpr (ACT < 0) {      // the input activation becomes a template argument
        if (a.elu) {
            if constexpr (!CT && KC == 16 && (KT == 1 || KT == 3)) return launch_conv_t<MT, KT, KC, CT, 4>(s, a, B, cfg);
            Q3_LOG("voc conv: ELU input is built for 1- and 3-tap convs at 16 channels per stage only");
            return -1;
        }
        if (a.alpha && a.gelu) {
            Q3_LOG("voc conv: Snake and GELU on one input are not built");
            return -1;
        }
        // (only the variant the long Snake 1 x 1 convs run is specialised: every further one is another kernel to compile)
        if constexpr (!(KT == 1 && KC == 16 && MT == 4 && !CT)) return launch_conv_t<MT, KT, KC, CT, 3>(s, a, B, cfg);
        else return a.alpha ? launch_conv_t<MT, KT, KC, CT, 1>(s, a, B, cfg) : a.gelu ? launch_conv_t<MT, KT, KC, CT, 2>(s, a, B, cfg)
                                                                             : launch_conv_t<MT, KT, KC, CT, 0>(s, a, B, cfg);
    } else {
    constexpr int TM = 32 * MT, TMP = voc_wpitch(TM);
    const int halo = (KT - 1) * a.dil;
    if (a.dil > 9) {
        Q3_LOG("voc conv: dilation %d > 9 is not built", a.dil);
        return -1;
    }
    size_t lds = ((size_t)KT * KC * TMP + (size_t)KC * voc_xpitch(VTN + ((halo + 3) & ~3))) * sizeof(float);
    if (CT && lds < (size_t)32 * (VTN + 1) * sizeof(float)) lds = (size_t)32 * (VTN + 1) * sizeof(float);   // store slab
    // experiment knob: Q3_VOC_LDS_PAD=bytes raises every conv launch's LDS request, i.e. lowers the vocoder's
    // residency per CU evenly (room for the frame loop's workgroups when the two run side by side)
    static const size_t lds_pad = getenv("Q3_VOC_LDS_PAD") ? (size_t)atol(getenv("Q3_VOC_LDS_PAD")) : 0;
    if (lds_pad > lds) {
        lds = lds_pad;
        static bool attr = false;
        if (!attr) {
            Q3_HIP(hipFuncSetAttribute((const void*)conv_kernel<MT, KT, KC, CT, ACT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), -1);
            attr = true;
        }
    }
    ConvArgs c = a;
    c.Mp = (a.M + 3) / 4 * 4;
    c.flat_B = (KT == 1 && a.stride == 1) ? B : 0;
    if ((a.ldx & 3) || (a.ldy & 3) || a.ldx < a.Lin || a.ldy < a.Lout || a.Lc < a.Lin || a.Lc > a.Lin + KT - 1) {
        Q3_LOG("voc conv: bad geometry (Lin %d pitch %d, Lout %d pitch %d, Lc %d)", a.Lin, a.ldx, a.Lout, a.ldy, a.Lc);
        return -1;
    }
    {   // the kernel indexes activations with 32-bit offsets from a.x / a.y (all chunks: the epilogue's `be` is per lane)
        if ((size_t)B * a.Cin * a.ldx >= ((size_t)1 << 31) || (size_t)B * a.Cout * a.ldy >= ((size_t)1 << 31)) {
            Q3_LOG("voc conv: activation of %d x %d x %d / %d x %d x %d floats is beyond the kernel's 32-bit indexing", B, a.Cin, a.ldx, B, a.Cout, a.ldy);
            return -1;
        }
    }
    c.tiles_l = ((c.flat_B > 0 ? a.ldx * B : a.Lc) + VTN - 1) / VTN;
    c.tiles_m = (a.M + TM - 1) / TM;
    c.n_tiles = c.tiles_l * c.tiles_m * (c.flat_B > 0 ? 1 : B);
    int grid = c.n_tiles;
    if (cfg.max_wgs > 0 && grid > cfg.max_wgs) grid = cfg.max_wgs;
    voc_note_variant(VV_CONV, MT, KT, KC, CT ? 1 : 0, ACT);
    hipLaunchKernelGGL((conv_kernel<MT, KT, KC, CT, ACT>), dim3(grid), dim3(256), lds, s, c);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
    }
}

template <int KT, int KC>
static int launch_conv_mt(hipStream_t s, const ConvArgs& a, int B, const VocSettings& cfg) {
    const int t32 = (a.M + 31) / 32;  // 32-row MFMA tiles needed
    int mt = 4;
    if (t32 % 4 != 0) mt = (t32 % 3 == 0) ? 3 : (t32 % 2 == 0) ? 2 : (t32 < 4 ? t32 : 4);
    // short activations (the 12.5 Hz / 25 Hz stages: 64-256 columns per chunk): tall tiles leave most CUs without a
    // workgroup (1024 -> 512 over 2048 columns is 4 x 16 = 64 tiles of 128 rows) -- take shorter tiles until the grid
    // covers the chip
    // covers the chip twice (measured, 32 chunks: pre-transformer 5.8 -> 4.2 ms, the 4096 -> 1024 ConvNeXt conv 0.83 -> 0.62)
    static const int fill_env = getenv("Q3_VOC_FILL") ? atoi(getenv("Q3_VOC_FILL")) : 512;
    const int fill = cfg.fill >= 0 ? cfg.fill : fill_env;
    if (fill > 0) {
        const long cols = (KT == 1 && a.stride == 1) ? (long)a.ldx * B : (long)a.Lc;
        const long col_tiles = (cols + VTN - 1) / VTN * ((KT == 1 && a.stride == 1) ? 1 : B);
        while (mt > 1 && col_tiles * ((t32 + mt - 1) / mt) < fill) mt = (mt == 4 || mt == 2) ? mt / 2 : 1;
    }
    switch (mt) {
        case 1: return launch_conv_t<1, KT, KC>(s, a, B, cfg);
        case 2: return launch_conv_t<2, KT, KC>(s, a, B, cfg);
        case 3: return launch_conv_t<3, KT, KC>(s, a, B, cfg);
        default: return launch_conv_t<4, KT, KC>(s, a, B, cfg);
    }
}

// ---------------------------------------------------------------------------
// The decoder's last conv: C channels -> ONE output row (7 taps, Snake on the input, clamp).  On the MFMA it is a
// 32-row tile with one live row (1.6 ms per 32 chunks at 0.97 TB/s); it is a dot product per sample and HBM-bound:
// each thread owns 8 consecutive samples, walks the channels, reads the 14 inputs they need as four aligned float4
// (neighbouring threads' overlap comes from L1), applies Snake once per input and accumulates the 7 taps in f32.
// Weights are read from conv_kernel's packed layout ([C/8][7][8][Mp], row 0) with wave-uniform (scalar) loads.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) conv_out1_kernel(ConvArgs a) {
    const int b = blockIdx.y;
    const int l0 = (blockIdx.x * 256 + threadIdx.x) * 8;
    if (l0 >= a.Lin) return;
    const float* xb = a.x + (size_t)b * a.Cin * a.ldx;
    float acc[8];
    const float b0 = a.bias ? a.bias[0] : 0.f;
#pragma unroll
    for (int j = 0; j < 8; j++) acc[j] = b0;
    for (int c = 0; c < a.Cin; c++) {
        const float* xr = xb + (size_t)c * a.ldx;      // (16-byte aligned: 4 | ldx)
        float v[16];   // columns l0 - 8 .. l0 + 7
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int l = l0 - 8 + 4 * q;
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
            if (l >= 0 && l + 3 < a.Lin) t = *(const float4*)(xr + l);
            else {
                if (l >= 0 && l < a.Lin) t.x = xr[l];
                if (l + 1 >= 0 && l + 1 < a.Lin) t.y = xr[l + 1];
                if (l + 2 >= 0 && l + 2 < a.Lin) t.z = xr[l + 2];
                if (l + 3 >= 0 && l + 3 < a.Lin) t.w = xr[l + 3];
            }
            v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
        }
        if (a.alpha) {   // Snake(0) = 0: the causal zero padding commutes with it
            const float al = a.alpha[c], ib = a.inv_beta[c];
#pragma unroll
            for (int i = 2; i < 16; i++) {
                const float sn = __sinf(al * v[i]);
                v[i] = v[i] + ib * (sn * sn);
            }
        }
        const float* wc = a.wk + (size_t)((c >> 3) * 7 * 8 + (c & 7)) * a.Mp;   // tap k: + k * 8 * Mp
#pragma unroll
        for (int k = 0; k < 7; k++) {
            const float wv = wc[(size_t)k * 8 * a.Mp];
#pragma unroll
            for (int j = 0; j < 8; j++) acc[j] = fmaf(wv, v[2 + j + k], acc[j]);   // tap k reads column l - (6 - k)
        }
    }
    float* yb = a.y + (size_t)b * a.ldy;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        float o = acc[j];
        if (a.clamp) o = fminf(fmaxf(o, -1.f), 1.f);
        if (l0 + j < a.Lin) yb[l0 + j] = o;
    }
}

int voc_launch_conv(hipStream_t s, const ConvArgs& a, int B, const VocSettings& cfg) {
    const int c = a.Cin;
    if (c % 8) {
        Q3_LOG("voc conv: Cin=%d is not a multiple of 8", c);
        return -1;
    }
    if (a.elu) {   // (ConvArgs::elu: one stage width, whatever the length or batch)
        if (c % 16 || (a.K != 1 && a.K != 3) || a.stride != 1 || a.alpha || a.gelu) {
            Q3_LOG("voc conv: ELU input needs a 1- or 3-tap stride-1 conv over a multiple of 16 channels (got %d taps, %d channels)", a.K, c);
            return -1;
        }
        return a.K == 1 ? launch_conv_mt<1, 16>(s, a, B, cfg) : launch_conv_mt<3, 16>(s, a, B, cfg);
    }
    static const int out1 = getenv("Q3_VOC_OUT1") ? atoi(getenv("Q3_VOC_OUT1")) : 1;
    if (out1 && a.M == 1 && a.K == 7 && a.dil == 1 && a.stride == 1 && !a.res && !a.gelu && (a.ldx & 3) == 0 &&
        (size_t)B * c * a.ldx < ((size_t)1 << 31)) {
        ConvArgs k = a;
        k.Mp = 4;
        voc_note_variant(VV_OUT1);
        hipLaunchKernelGGL(conv_out1_kernel, dim3((a.Lin + 2047) / 2048, B), dim3(256), 0, s, k);
        Q3_HIP(hipGetLastError(), -1);
        return 0;
    }
    // one / two taps: 16-channel stages (the one-tap form prefetches the next stage's operands into registers; the
    // 32-channel variants of the 128-row tile spill 27-35 registers).  Measured at 32 chunks: 384 -> 384 k1 1.74 -> 1.28 ms,
    // 768 -> 768 k1 1.06 -> 0.84, the ConvNeXt 1024 -> 4096 convs 0.39 / 0.74 -> 0.35 / 0.64; Q3_VOC_KC_MAX=32 restores
    // the 32-channel stages (channel counts that are no multiple of 16 take them or the 8-channel ones anyway).
    // Short activations (the 12.5 / 25 / 50 Hz stages: <= 512 columns per chunk) are the other way round: their tiles are
    // 32-64 rows (launch_conv_mt shrinks them until the grid covers the chip), a stage is a handful of MFMAs, and the
    // barrier pair per stage is what they pay for -- 32-channel stages there (round 3, per-op profile at 32 chunks:
    // the pre-transformer's 1024 -> 512 projections 69-75 -> 58 us, ConvNeXt 4096 -> 1024 0.60 / 0.88 -> 0.56 / 0.83 ms).
    static const int kc_max = getenv("Q3_VOC_KC_MAX") ? atoi(getenv("Q3_VOC_KC_MAX")) : 16;
    // (the rule looks at ONE chunk's columns, never at the batch: a chunk must decode to the same bits alone and inside a
    // batch, and with two taps the stage width changes the order in which taps and channels are summed)
    const bool short_act = (a.Lrule > 0 ? a.Lrule : a.Lc) <= 512 && a.M <= 4096 && c % 32 == 0 && a.K <= 2;   // (not the 1536 -> 768 x 8 transposed conv: 2.92 -> 3.10 ms)
    if (kc_max < 32 && !short_act && c % 16 == 0 && (a.K == 1 || a.K == 2))
        return a.K == 1 ? launch_conv_mt<1, 16>(s, a, B, cfg) : launch_conv_mt<2, 16>(s, a, B, cfg);
    switch (a.K) {
        case 1: return c % 32 == 0 ? launch_conv_mt<1, 32>(s, a, B, cfg) : c % 16 == 0 ? launch_conv_mt<1, 16>(s, a, B, cfg) : launch_conv_mt<1, 8>(s, a, B, cfg);
        case 2: return c % 32 == 0 ? launch_conv_mt<2, 32>(s, a, B, cfg) : c % 16 == 0 ? launch_conv_mt<2, 16>(s, a, B, cfg) : launch_conv_mt<2, 8>(s, a, B, cfg);
        case 3: return c % 16 == 0 ? launch_conv_mt<3, 16>(s, a, B, cfg) : launch_conv_mt<3, 8>(s, a, B, cfg);
        case 7: return launch_conv_mt<7, 8>(s, a, B, cfg);
        default:
            Q3_LOG("voc conv: kernel with %d taps is not built (1, 2, 3, 7 are)", a.K);
            return -1;
    }
}

// ---------------------------------------------------------------------------
// Fused residual unit of the decoder blocks at 96 / 192 channels (the two HBM-bound stages):
//     y = x + conv1x1(Snake_b(conv7_dilated(Snake_a(x))))
// in ONE launch.  The 7-tap conv's accumulators never leave the registers: the MFMA's D layout holds, per lane,
// one column and 16 channels of each 32-row tile -- exactly a B operand of the 1x1 conv if its K axis is walked
// in the order (tile, register): step t = (mt, q) contracts channel 32 mt + (q & 3) + 8 (q >> 2) in lanes 0-31
// and that channel + 4 in lanes 32-63.  The 1x1 weights are stored at load time in that order as the matching A
// operands (w1p[row tile][t][lane]), so the second GEMM is `mfma(Ws[t*64 + lane], acc1[mt][q], acc2)`.
// HBM traffic per unit: x once (+ halo), y once -- against x, the copy kept for the residual (read + write), the
// 7-tap output (write + read), the residual read and y for the three launches it replaces.
template <int MT>
__global__ void __launch_bounds__(256, MT <= 3 ? 3 : 2) resunit_kernel(ResUnitArgs a) {
    constexpr int C = 32 * MT, KT = 7, KC = 8, TMP = voc_wpitch(C);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int halo = (KT - 1) * a.dil, HA = (halo + 3) & ~3, XW = VTN + HA, XP = voc_xpitch(XW);   // (conv_kernel: float4 staging)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Ws = lds;                   // [KT][KC][TMP]; later one row tile of the 1x1 weights [C/2][64]
    float* Xs = lds + KT * KC * TMP;   // [KC][XP]
    float* Ps = Xs + KC * XP;          // [4][C]: b7, al1, ib1, b1
    for (int i = tid; i < C; i += 256) {
        Ps[i] = a.b7 ? a.b7[i] : 0.f;
        Ps[C + i] = a.al1[i];
        Ps[2 * C + i] = a.ib1[i];
        Ps[3 * C + i] = a.b1 ? a.b1[i] : 0.f;
    }
    for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const int lx = tile % a.tiles_l, b = tile / a.tiles_l;
        const int l0 = lx * VTN;
        const float* xb = a.x + (size_t)b * C * a.ld;
        f16v acc[MT];
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int i = 0; i < 16; i++) acc[mt][i] = 0.f;
        // ---- the dilated 7-tap conv (same staging and MFMA loop as conv_kernel<MT, 7, 8> over all C rows) ----
        for (int ci0 = 0; ci0 < C; ci0 += KC) {
            __syncthreads();
            constexpr int WN = KT * KC * (C / 4), WIT = (WN + 255) / 256;
            float4 wv[WIT];
#pragma unroll
            for (int i = 0; i < WIT; i++) {
                const int idx = tid + i * 256, ic = idx < WN ? idx : 0;
                const int m4 = ic % (C / 4), ci = (ic / (C / 4)) % KC, k = ic / ((C / 4) * KC);
                const int cg = ci0 + ci;
                wv[i] = *(const float4*)(a.w7 + (unsigned)((((cg >> 3) * KT + k) * 8 + (cg & 7)) * C + m4 * 4));
            }
            constexpr int LPC = 256 / KC, XG = (VTN + (((KT - 1) * 9 + 3) & ~3)) / 4, XJ = (XG + LPC - 1) / LPC;
            const int xci = tid / LPC, xl = tid - xci * LPC;
            const float al = a.al7[ci0 + xci], ib = a.ib7[ci0 + xci];
            float4 xv[XJ];
#pragma unroll
            for (int j = 0; j < XJ; j++) {
                const int c4 = (xl + j * LPC) * 4;
                const int l = l0 - HA + c4, lc = (c4 < XW && l >= 0 && l < a.Lin) ? l : 0;
                xv[j] = *(const float4*)(xb + (unsigned)((ci0 + xci) * a.ld + lc));
            }
#pragma unroll
            for (int i = 0; i < WIT; i++) {
                const int idx = tid + i * 256;
                if (idx < WN) {
                    const int m4 = idx % (C / 4), ci = (idx / (C / 4)) % KC, k = idx / ((C / 4) * KC);
                    *(float4*)(Ws + (k * KC + ci) * TMP + m4 * 4) = wv[i];
                }
            }
#pragma unroll
            for (int j = 0; j < XJ; j++) {
                const int c4 = (xl + j * LPC) * 4;
                if (c4 < XW) {
                    const int l = l0 - HA + c4;
                    float4 v = xv[j];
                    float sn;
                    sn = __sinf(al * v.x); v.x = v.x + ib * (sn * sn);
                    sn = __sinf(al * v.y); v.y = v.y + ib * (sn * sn);
                    sn = __sinf(al * v.z); v.z = v.z + ib * (sn * sn);
                    sn = __sinf(al * v.w); v.w = v.w + ib * (sn * sn);
                    if (l < 0) v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (l >= a.Lin) v.x = 0.f;
                    if (l + 1 >= a.Lin) v.y = 0.f;
                    if (l + 2 >= a.Lin) v.z = 0.f;
                    if (l + 3 >= a.Lin) v.w = 0.f;
                    *(float4*)(Xs + xci * XP + c4) = v;
                }
            }
            __syncthreads();
#pragma unroll 1
            for (int k = 0; k < KT; k++) {
                const int off = HA - (KT - 1 - k) * a.dil + w * 32 + (lane & 31);
#pragma unroll
                for (int kk = 0; kk < KC; kk += 2) {
                    const int ci = kk + (lane >> 5);
                    const float bv = Xs[ci * XP + off];
#pragma unroll
                    for (int mt = 0; mt < MT; mt++) {
                        const float av = Ws[(k * KC + ci) * TMP + mt * 32 + (lane & 31)];
                        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[mt], 0, 0, 0);
                    }
                }
            }
        }
        // ---- bias + Snake on the accumulators: they become the 1x1 conv's B operands in place ----
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int c = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                const float v = acc[mt][r] + Ps[c];
                const float sn = __sinf(Ps[C + c] * v);
                acc[mt][r] = v + Ps[2 * C + c] * (sn * sn);
            }
        // ---- the 1x1 conv, one 32-row output tile at a time, + bias + residual ----
        const int gl = l0 + w * 32 + (lane & 31);
        const bool live = gl < a.Lin;
#pragma unroll 1
        for (int mt2 = 0; mt2 < MT; mt2++) {
            // element (row m, column gl): the row splits into a wave-uniform part (32 mt2 + the register's row: scalar
            // address arithmetic) and ONE per-lane offset; written as 16 per-lane offsets the compiler computed all of
            // them (and the 16 of the stores) at kernel entry and spilled them (36 registers, round 2)
            const unsigned lane_off = (unsigned)(4 * (lane >> 5) * a.ld + (live ? gl : 0));
            float res[16];
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const float* rowp = xb + (unsigned)((32 * mt2 + (r & 3) + 8 * (r >> 2)) * a.ld);
                res[r] = rowp[lane_off];
            }
            __syncthreads();   // the 7-tap stage (or the previous row tile) is consumed by every wave
#pragma unroll
            for (int i = 0; i < MT; i++) {   // 32 C floats = 8 C float4 = MT per thread
                const int idx = tid + i * 256;
                *(float4*)(Ws + idx * 4) = *(const float4*)(a.w1p + (unsigned)(mt2 * 32 * C + idx * 4));
            }
            __syncthreads();
            f16v o;
#pragma unroll
            for (int i = 0; i < 16; i++) o[i] = 0.f;
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
#pragma unroll
                for (int q = 0; q < 16; q++)
                    o = __builtin_amdgcn_mfma_f32_32x32x2f32(Ws[(mt * 16 + q) * 64 + lane], acc[mt][q], o, 0, 0, 0);
            if (live) {
                float* yb = a.y + (size_t)b * C * a.ld;
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int mu = 32 * mt2 + (r & 3) + 8 * (r >> 2);
                    float* rowp = yb + (unsigned)(mu * a.ld);
                    __builtin_nontemporal_store(o[r] + Ps[3 * C + mu + 4 * (lane >> 5)] + res[r], &rowp[lane_off]);
                }
            }
        }
    }
}

template <int MT>
static int launch_resunit_t(hipStream_t s, ResUnitArgs a, int B, const VocSettings& cfg) {
    constexpr int C = 32 * MT;
    const int halo = 6 * a.dil;
    if (a.dil > 9) return -1;
    const size_t lds = ((size_t)7 * 8 * voc_wpitch(C) + (size_t)8 * voc_xpitch(VTN + ((halo + 3) & ~3)) + 4 * C) * sizeof(float);
    a.tiles_l = (a.Lin + VTN - 1) / VTN;
    a.n_tiles = a.tiles_l * B;
    int grid = a.n_tiles;
    if (cfg.max_wgs > 0 && grid > cfg.max_wgs) grid = cfg.max_wgs;
    voc_note_variant(VV_RESUNIT, MT);
    hipLaunchKernelGGL((resunit_kernel<MT>), dim3(grid), dim3(256), lds, s, a);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

bool resunit_channels(int c) { return c == 96 || c == 192; }

int launch_resunit(hipStream_t s, const ResUnitArgs& a, int C, int B, const VocSettings& cfg) {
    return C == 96 ? launch_resunit_t<3>(s, a, B, cfg) : C == 192 ? launch_resunit_t<6>(s, a, B, cfg) : -1;
}

// ---------------------------------------------------------------------------
// Split-precision path: fp32-grade products on the fp16 MFMA (16x the rate of the exact-fp32 MFMA).
// Every operand v is carried as two fp16 terms: hi = fp16(v), lo = fp16((v - hi) * 2048) (22 mantissa bits
// together; the scale keeps lo out of the subnormals).  a*b ~= hi_a*hi_b + (hi_a*lo_b + lo_a*hi_b)/2048:
// three v_mfma_f32_32x32x16_f16 with f32 accumulation (products of fp16 values are exact in f32); the
// dropped lo*lo term is 2^-22 relative.  Measured against a float64 evaluation of the same table the result
// is as close as the exact-fp32 MFMA path and torch's CPU fp32 (2e-7 of full scale; tests/test_gpu_vocoder.py).
//   snake_split_kernel  x f32 [B][C][L] -> Snake -> hi/lo planes fp16 [B][C/8][L][8] (8-channel groups,
//                       channel-minor: one 16-B record = one lane's MFMA B operand; a conv stage's input tile
//                       is two contiguous runs, a tap a row shift; the producing conv's epilogue writes whole
//                       records with lanes l, l+32 side by side)
//   conv_split_kernel   implicit GEMM, K dimension = 16 input channels per MFMA; weights split once at load
//                       into [Cin/16][tap][rows][16] planes.  Workgroup = 64 rows x 256 columns, 4 waves side
//                       by side (64 x 64 each: all share the weight fragments); staging is pure 16-B copies.
// ---------------------------------------------------------------------------
typedef _Float16 hv8 __attribute__((ext_vector_type(8)));

__global__ void __launch_bounds__(256) snake_split_kernel(const float* __restrict__ x, const float* __restrict__ alpha,
                                                          const float* __restrict__ inv_beta, _Float16* __restrict__ xh,
                                                          _Float16* __restrict__ xl, int C, int L, int ld, int gelu,
                                                          int* __restrict__ ovf, int ovf_stride) {
    const int l = blockIdx.x * 256 + threadIdx.x, cg = blockIdx.y, b = blockIdx.z;   // cg: 8-channel group
    if (l >= L) return;
    const float* xp = x + ((size_t)b * C + cg * 8) * ld + l;     // f32 rows at pitch ld; the planes are dense in L
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = xp[(size_t)j * ld];
    if (alpha) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float sn = __sinf(alpha[cg * 8 + j] * v[j]);
            v[j] = v[j] + inv_beta[cg * 8 + j] * (sn * sn);
        }
    }
    if (gelu) {
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = gelu_erf(v[j]);
    }
    hv8 h, lo;
    bool big = false;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        big |= !(fabsf(v[j]) <= 65504.f);   // beyond the hi term's range (or NaN): the split form cannot carry it
        const _Float16 hi = (_Float16)fminf(fmaxf(v[j], -65504.f), 65504.f);
        h[j] = hi;
        lo[j] = (_Float16)((v[j] - (float)hi) * 2048.0f);
    }
    const size_t o = (((size_t)b * (C >> 3) + cg) * L + l) * 8;
    *(hv8*)(xh + o) = h;
    *(hv8*)(xl + o) = lo;
    if (big) ovf[(size_t)b * ovf_stride] = 1;   // (stride 0: one flag for the call)
}

int voc_launch_snake_split(hipStream_t s, const float* x, const float* alpha, const float* inv_beta, _Float16* xh, _Float16* xl, int C,
                           int L, int ld, int gelu, int* ovf, int B, int ovf_stride) {
    voc_note_variant(VV_SNAKE_SPLIT);
    hipLaunchKernelGGL(snake_split_kernel, dim3((unsigned)((L + 255) / 256), C / 8, B), dim3(256), 0, s, x, alpha, inv_beta, xh, xl, C, L, ld,
                       gelu, ovf, ovf_stride);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}
constexpr int SKC = 16;  // input channels per k-step

// KT taps; KS 16-channel k-steps per LDS stage (few-tap convs stage several, so a barrier pair buys more MFMAs);
// MW 32-row MFMA tiles per workgroup (rows = 32*MW: 96 divides every channel count of the decoder, so the
// input tile is read by Cout/96 workgroups instead of Cout/64 and no row is padding)
// NJ 32-column tiles per wave (workgroup = 4 waves side by side = 128*NJ columns): 2 for the MFMA-bound layers,
// 1 for the few-tap HBM-bound ones, whose half-size accumulators let a third workgroup per CU overlap the phases
template <int KT, int KS, int MW, int NJ>
__global__ void __launch_bounds__(256, NJ == 1 ? 3 : 2) conv_split_kernel(SplitArgs a) {
    constexpr int STM = 32 * MW, STN = 128 * NJ;
    constexpr int UNR = (MW == 3 && KT == 7) ? 1 : KS * KT;   // unroll of the tap loop
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int halo = (KT - 1) * a.dil;
    const int XW = STN + halo;
    extern __shared__ __attribute__((aligned(16))) char slds[];
    _Float16* Wh = (_Float16*)slds;                    // [KS][KT][STM][16]
    _Float16* Wl = Wh + KS * KT * STM * SKC;
    _Float16* Xh = Wl + KS * KT * STM * SKC;           // [KS][2][XW][8]: per k-step its two 8-channel groups
    _Float16* Xl = Xh + (size_t)KS * XW * SKC;
    const int C16 = a.Cin >> 4;
    const hv8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    // Tile order.  Big weights (my_fast = 0): columns fastest, then chunk, row tile slowest -- at any moment the
    // chip works on one or two row tiles, whose weights stay in every XCD's L2 while the input tiles stream.
    // Small weights (my_fast = 1, they fit every L2 whole): XCD x (= workgroup id mod 8 under round-robin
    // placement) owns the column tiles x, x+8, ... and walks each one's row tiles back to back, so the input
    // tile comes from HBM once and from that XCD's L2 for the other row tiles.
    for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        int lx, b, my;
        if (a.my_fast) {
            const int xcd = tile & 7, j = tile >> 3;
            my = j % a.tiles_m;
            const int cg = (j / a.tiles_m) * 8 + xcd;
            if (cg >= a.tiles_l * a.B) continue;
            lx = cg % a.tiles_l;
            b = cg / a.tiles_l;
        } else {
            lx = tile % a.tiles_l;
            b = (tile / a.tiles_l) % a.B;
            my = tile / (a.tiles_l * a.B);
        }
        const int l0 = lx * STN, m0 = my * STM;
        f16v acc[MW][NJ], accx[MW][NJ];
#pragma unroll
        for (int i = 0; i < MW; i++)
#pragma unroll
            for (int j = 0; j < NJ; j++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    acc[i][j][r] = 0.f;
                    accx[i][j][r] = 0.f;
                }
        for (int cb = 0; cb < C16; cb += KS) {
            __syncthreads();
            // weights: per (k-step, tap) one contiguous 2 KiB run of each plane
            for (int idx = tid; idx < KS * KT * STM * 2; idx += 256) {      // 16-byte pieces
                const int sk = idx / (STM * 2), rem = idx - sk * (STM * 2);      // sk = ks*KT + k
                const size_t g = ((size_t)(cb * KT + sk) * a.Mp + m0) * SKC + rem * 8;
                *(hv8*)(Wh + idx * 8) = *(const hv8*)(a.w_hi + g);
                *(hv8*)(Wl + idx * 8) = *(const hv8*)(a.w_lo + g);
            }
            // input: columns l0-halo .. l0+255 of the stage's 2*KS 8-channel groups, one contiguous run each
            for (int idx = tid; idx < KS * 2 * XW; idx += 256) {
                const int grp = idx / XW, col = idx - grp * XW;
                const int l = l0 - halo + col;
                hv8 vh = zero8, vl = zero8;
                if (l >= 0 && l < a.Lin) {
                    const size_t g = ((((size_t)b * C16 + cb) * 2 + grp) * a.Lin + l) * 8;
                    vh = *(const hv8*)(a.xh + g);
                    vl = *(const hv8*)(a.xl + g);
                }
                *(hv8*)(Xh + idx * 8) = vh;
                *(hv8*)(Xl + idx * 8) = vl;
            }
            __syncthreads();
            // the 96-row 7-tap form sits at the 256-register limit: walking its taps one at a time keeps it from spilling
#pragma unroll UNR
            for (int sk = 0; sk < KS * KT; sk++) {
                const int ks = sk / KT, k = sk % KT;
                const int off = k * a.dil;   // tap k reads column l - (KT-1-k)*dil = staged column (l-l0) + k*dil
                hv8 ah[MW], al[MW], bh[NJ], bl[NJ];
#pragma unroll
                for (int i = 0; i < MW; i++) {
                    const int row = i * 32 + (lane & 31);
                    ah[i] = *(const hv8*)(Wh + (sk * STM + row) * SKC + (lane >> 5) * 8);
                    al[i] = *(const hv8*)(Wl + (sk * STM + row) * SKC + (lane >> 5) * 8);
                }
#pragma unroll
                for (int i = 0; i < NJ; i++) {
                    const int col = w * (32 * NJ) + i * 32 + (lane & 31) + off;
                    bh[i] = *(const hv8*)(Xh + ((size_t)(ks * 2 + (lane >> 5)) * XW + col) * 8);
                    bl[i] = *(const hv8*)(Xl + ((size_t)(ks * 2 + (lane >> 5)) * XW + col) * 8);
                }
#pragma unroll
                for (int i = 0; i < MW; i++)
#pragma unroll
                    for (int j = 0; j < NJ; j++) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
                        accx[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bl[j], accx[i][j], 0, 0, 0);
                        accx[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bh[j], accx[i][j], 0, 0, 0);
                    }
            }
        }
        typedef _Float16 hv4 __attribute__((ext_vector_type(4)));
#pragma unroll
        for (int i = 0; i < MW; i++)
#pragma unroll
            for (int j = 0; j < NJ; j++) {
                const int l = l0 + w * (32 * NJ) + j * 32 + (lane & 31);
                if (l < a.Lc) {
                    float rv[16];
#pragma unroll
                    for (int r = 0; r < 16; r++) {     // the residual reads of the whole 32x32 tile go out together
                        const int m = m0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                        rv[r] = 0.f;
                        if (a.res && m < a.M) {
                            const int co = a.stride == 1 ? m : m / a.stride;
                            const int p = a.stride == 1 ? 0 : m % a.stride;
                            rv[r] = a.res[((size_t)b * a.Cout + co) * a.ldy + (size_t)l * a.stride + p];   // (stride 1 only)
                        }
                    }
#pragma unroll
                    for (int g = 0; g < 4; g++) {      // accumulator registers 4g..4g+3 = 4 consecutive rows
                        const int mg = m0 + i * 32 + 8 * g + 4 * (lane >> 5);
                        float v[4];
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            const int m = mg + q, r = 4 * g + q;
                            v[q] = acc[i][j][r] + accx[i][j][r] * (1.0f / 2048.0f);
                            if (m < a.M) {
                                const int co = a.stride == 1 ? m : m / a.stride;
                                const int p = a.stride == 1 ? 0 : m % a.stride;
                                const int jo = l * a.stride + p - a.lt;          // output column after the left trim
                                const size_t idx = ((size_t)b * a.Cout + co) * a.ldy + (size_t)(jo > 0 ? jo : 0);
                                if (a.bias) v[q] += a.bias[co];
                                v[q] += rv[r];
                                if (a.clamp) v[q] = fminf(fmaxf(v[q], -1.f), 1.f);
                                if (a.y && jo >= 0 && jo < a.Lout) a.y[idx] = v[q];
                            }
                        }
                        if (a.oh && mg < a.M) {
                            hv4 vh, vl;
                            bool big = false;
#pragma unroll
                            for (int q = 0; q < 4; q++) {
                                float t = v[q];
                                if (a.oalpha) {
                                    const float sn = __sinf(a.oalpha[mg + q] * t);
                                    t = t + a.oinv_beta[mg + q] * (sn * sn);
                                }
                                big |= !(fabsf(t) <= 65504.f);
                                const _Float16 hi = (_Float16)fminf(fmaxf(t, -65504.f), 65504.f);
                                vh[q] = hi;
                                vl[q] = (_Float16)((t - (float)hi) * 2048.0f);
                            }
                            if (big) a.ovf[(size_t)b * a.ovf_stride] = 1;
                            const size_t o = (((size_t)b * (a.Cout >> 3) + (mg >> 3)) * a.Lin + l) * 8 + (mg & 7);
                            *(hv4*)(a.oh + o) = vh;
                            *(hv4*)(a.ol + o) = vl;
                        }
                    }
                }
            }
    }
}

template <int KT, int KS, int MW, int NJ>
static int launch_conv_split_t(hipStream_t s, const SplitArgs& a, int B, const VocSettings& cfg) {
    constexpr int STM = 32 * MW, STN = 128 * NJ;
    if (a.dil > 9) return -1;
    const int halo = (KT - 1) * a.dil;
    const size_t lds = ((size_t)2 * KS * KT * STM * SKC + (size_t)2 * KS * (STN + halo) * SKC) * sizeof(_Float16);
    static bool set_ = false;
    if (!set_) {
        Q3_HIP(hipFuncSetAttribute((const void*)conv_split_kernel<KT, KS, MW, NJ>, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024), -1);
        set_ = true;
    }
    if (lds > 80 * 1024 || (a.Cin / 16) % KS || a.Mp % STM) return -1;   // <= 80 KB: two workgroups per CU
    SplitArgs c = a;
    c.B = B;
    c.tiles_l = (a.Lc + STN - 1) / STN;
    c.tiles_m = (a.M + STM - 1) / STM;
    c.n_tiles = c.tiles_l * c.tiles_m * B;
    // both planes of all taps of the weights: small enough to live in every XCD's 4 MiB L2 beside the stream?
    c.my_fast = c.tiles_m > 1 && (size_t)a.Cin * a.Mp * KT * 4 <= (size_t)2 << 20;
    if (c.my_fast) c.n_tiles = (c.tiles_l * B + 7) / 8 * 8 * c.tiles_m;
    int grid = c.n_tiles;
    if (cfg.max_wgs > 0 && grid > cfg.max_wgs) grid = cfg.max_wgs;
    voc_note_variant(VV_SPLIT, KT, KS, MW, NJ, c.my_fast);
    hipLaunchKernelGGL((conv_split_kernel<KT, KS, MW, NJ>), dim3(grid), dim3(256), lds, s, c);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

template <int MW>
static int launch_conv_split_m(hipStream_t s, const SplitArgs& a, int K, int B, const VocSettings& cfg) {
    const int c16 = a.Cin / 16;
    switch (K) {
        case 1:
            if (cfg.narrow_k1 && MW == 3)
                return c16 % 3 == 0 ? launch_conv_split_t<1, 3, MW, 1>(s, a, B, cfg) : c16 % 2 == 0 ? launch_conv_split_t<1, 2, MW, 1>(s, a, B, cfg) : launch_conv_split_t<1, 1, MW, 1>(s, a, B, cfg);
            return c16 % 3 == 0 ? launch_conv_split_t<1, 3, MW, 2>(s, a, B, cfg) : c16 % 2 == 0 ? launch_conv_split_t<1, 2, MW, 2>(s, a, B, cfg) : launch_conv_split_t<1, 1, MW, 2>(s, a, B, cfg);
        case 2:
            if (cfg.narrow_k1 && MW == 3 && a.Cin <= 384)   // the HBM-bound transposed convs (measured: 1536 -> 768 loses)
                return c16 % 2 == 0 ? launch_conv_split_t<2, 2, MW, 1>(s, a, B, cfg) : launch_conv_split_t<2, 1, MW, 1>(s, a, B, cfg);
            return c16 % 2 == 0 ? launch_conv_split_t<2, 2, MW, 2>(s, a, B, cfg) : launch_conv_split_t<2, 1, MW, 2>(s, a, B, cfg);
        case 3: return c16 % 2 == 0 && MW == 2 ? launch_conv_split_t<3, 2, MW, 2>(s, a, B, cfg) : launch_conv_split_t<3, 1, MW, 2>(s, a, B, cfg);
        case 7:
            if (cfg.narrow_k1 && a.Cin <= 192) return launch_conv_split_t<7, 1, MW, 1>(s, a, B, cfg);   // the HBM-bound blocks: -4..9 %
            return launch_conv_split_t<7, 1, MW, 2>(s, a, B, cfg);
        default: return -1;
    }
}

int launch_conv_split(hipStream_t s, const SplitArgs& a, int K, int B, const VocSettings& cfg) {
    // 96-row tiles where they tile the rows exactly (every channel count of the decoder blocks) and still
    // give the chip enough workgroups: the input tile is read by Cout/96 workgroups instead of Cout/64
    const long tiles96 = (long)((a.Lc + 255) / 256) * (a.M / 96) * B;
    const bool fits96 = a.M % 96 == 0 && a.Mp % 96 == 0;
    const bool use96 = fits96 && (a.Mp % 64 != 0 || tiles96 >= (cfg.fill >= 0 ? cfg.fill : 512));
    return use96 ? launch_conv_split_m<3>(s, a, K, B, cfg) : launch_conv_split_m<2>(s, a, K, B, cfg);
}

// ---------------------------------------------------------------------------
// The small f32 ops of the published decoder's transformer / ConvNeXt stages (activations [B][C][L], L <= a few
// hundred columns: latency-sized kernels, one thread per output or per column).
// ---------------------------------------------------------------------------
// causal depthwise conv: y[c][l] = bias[c] + sum_k w[c][k] * x[c][l - (K-1-k)]
__global__ void __launch_bounds__(256) dwconv_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                     const float* __restrict__ bias, float* __restrict__ y, int C, int L, int ld, int K) {
    const int l = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
    if (l >= L) return;
    const float* xr = x + ((size_t)b * C + c) * ld;
    float acc = bias ? bias[c] : 0.f;
    for (int k = 0; k < K; k++) {
        const int ls = l - (K - 1 - k);
        if (ls >= 0) acc += w[c * K + k] * xr[ls];
    }
    y[((size_t)b * C + c) * ld + l] = acc;
}

int voc_launch_dwconv(hipStream_t s, const float* x, const float* w, const float* bias, float* y, int C, int L, int ld, int K, int B) {
    hipLaunchKernelGGL(dwconv_kernel, dim3((unsigned)((L + 255) / 256), C, B), dim3(256), 0, s, x, w, bias, y, C, L, ld, K);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

// RMSNorm (kind 0) / LayerNorm (kind 1) over the channels of every column.  Workgroup = 64 columns x 16 channel
// lanes: a wave reads 64 consecutive columns of one channel (coalesced), the 16 partial sums of a column meet in LDS.
// Two-pass variance (mean first), like the reference implementation.
__global__ void __launch_bounds__(1024) chan_norm_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ bias, float* __restrict__ y, int C, int L,
                                                         int ld, int kind, float eps) {
    __shared__ float part[16][64];
    const int col = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int l = blockIdx.x * 64 + col, b = blockIdx.y;
    const bool ok = l < L;
    const float* xc = x + (size_t)b * C * ld + (ok ? l : 0);
    auto column_sum = [&](float v) -> float {     // sum over the 16 channel lanes of a column, identical in all of them
        part[g][col] = v;
        __syncthreads();
        float s_ = 0.f;
#pragma unroll
        for (int i = 0; i < 16; i++) s_ += part[i][col];
        __syncthreads();
        return s_;
    };
    float mu = 0.f;
    if (kind == 1) {
        float s_ = 0.f;
        for (int c = g; c < C; c += 16) s_ += xc[(size_t)c * ld];
        mu = column_sum(s_) / (float)C;
    }
    float ss = 0.f;
    for (int c = g; c < C; c += 16) {
        const float d = xc[(size_t)c * ld] - mu;
        ss += d * d;
    }
    const float inv = 1.0f / sqrtf(column_sum(ss) / (float)C + eps);
    if (!ok) return;
    float* yc = y + (size_t)b * C * ld + l;
    for (int c = g; c < C; c += 16) {
        float v = (xc[(size_t)c * ld] - mu) * inv * w[c];
        if (bias) v += bias[c];
        yc[(size_t)c * ld] = v;
    }
}

// x = [q | k | v] (head-major channels, [3*H*D][L]) -> causal sliding-window attention with rotate-half RoPE
// (positions = columns of the chunk).  One wave per (query column, head); lane j owns the pair (j, j + D/2).
__global__ void __launch_bounds__(64) voc_attn_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int D, int Lv,
                                                      int L, int window, float theta) {
    // L: row pitch (every row index below is scaled by it); Lv valid columns = the grid's x extent
    const int i = blockIdx.x, h = blockIdx.y, b = blockIdx.z, j = threadIdx.x;
    const int half = D / 2, HD = H * D;
    const bool on = j < half;
    const float* xb = x + (size_t)b * 3 * HD * L;
    const float inv_freq = on ? __powf(theta, -2.0f * (float)j / (float)D) : 0.f;
    auto rope = [&](const float* base, int pos, float& a, float& c) {   // rows (j, j+half) of a head at column pos
        float x0 = 0.f, x1 = 0.f;
        if (on) {
            x0 = base[(size_t)j * L + pos];
            x1 = base[(size_t)(j + half) * L + pos];
        }
        float sn, cs;
        __sincosf((float)pos * inv_freq, &sn, &cs);
        a = x0 * cs - x1 * sn;
        c = x1 * cs + x0 * sn;
    };
    float q0, q1;
    rope(xb + (size_t)(h * D) * L, i, q0, q1);
    const float scale = 1.0f / sqrtf((float)D);
    float m = -INFINITY, lsum = 0.f, o0 = 0.f, o1 = 0.f;
    const int t0 = i - window + 1 > 0 ? i - window + 1 : 0;
    for (int t = t0; t <= i; t++) {
        float k0, k1;
        rope(xb + (size_t)(HD + h * D) * L, t, k0, k1);
        float sc = q0 * k0 + q1 * k1;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sc += __shfl_xor(sc, o, 64);
        sc *= scale;
        const float mn = fmaxf(m, sc), corr = __expf(m - mn), p = __expf(sc - mn);
        float v0 = 0.f, v1 = 0.f;
        if (on) {
            const float* vb = xb + (size_t)(2 * HD + h * D) * L;
            v0 = vb[(size_t)j * L + t];
            v1 = vb[(size_t)(j + half) * L + t];
        }
        lsum = lsum * corr + p;
        o0 = o0 * corr + p * v0;
        o1 = o1 * corr + p * v1;
        m = mn;
    }
    if (on) {
        float* yb = y + ((size_t)b * HD + h * D) * L;
        yb[(size_t)j * L + i] = o0 / lsum;
        yb[(size_t)(j + half) * L + i] = o1 / lsum;
    }
}

// The same attention for a chunk whose q, k, v of one head fit in LDS (3 * L * D floats <= 64 KiB: the 64-column
// chunks of the pre-transformer): one workgroup per (head, chunk) applies RoPE once per element while staging, then
// every query is owned by 4 threads that split its keys 4 ways (online softmax each, merged by shuffles).
__global__ void __launch_bounds__(256) voc_attn_tile_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int D,
                                                            int L, int ld, int window, float theta) {
    extern __shared__ float sm[];            // q[L][D+1] | k[L][D+1] | v[L][D+1]  (+1: conflict-free row walks)
    const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int half = D / 2, HD = H * D, DP = D + 1;
    float *qs = sm, *ks = sm + (size_t)L * DP, *vs = sm + (size_t)2 * L * DP;
    const float* xb = x + (size_t)b * 3 * HD * ld;
    // stage: element (d, l) of q / k rotated with its partner (d +- half, l); consecutive threads = consecutive l
    for (int idx = tid; idx < half * L; idx += 256) {
        const int j = idx / L, l = idx - j * L;
        float sn, cs;
        __sincosf((float)l * __powf(theta, -2.0f * (float)j / (float)D), &sn, &cs);
#pragma unroll
        for (int which = 0; which < 2; which++) {
            const float* base = xb + (size_t)(which * HD + h * D) * ld;
            const float x0 = base[(size_t)j * ld + l], x1 = base[(size_t)(j + half) * ld + l];
            float* dst = which == 0 ? qs : ks;
            dst[l * DP + j] = x0 * cs - x1 * sn;
            dst[l * DP + j + half] = x1 * cs + x0 * sn;
        }
    }
    for (int idx = tid; idx < D * L; idx += 256) {
        const int d = idx / L, l = idx - d * L;
        vs[l * DP + d] = xb[(size_t)(2 * HD + h * D + d) * ld + l];
    }
    __syncthreads();
    const float scale = 1.0f / sqrtf((float)D);
    for (int i0 = 0; i0 < L; i0 += 64) {       // 64 queries per round: thread = (query, key lane)
        const int i = i0 + (tid >> 2), kl = tid & 3;
        float m = -INFINITY, lsum = 0.f;
        float o[64];                            // D <= 64 on this path
#pragma unroll
        for (int d = 0; d < 64; d++) o[d] = 0.f;
        if (i < L) {
            const int t0 = i - window + 1 > 0 ? i - window + 1 : 0;
            for (int t = t0 + kl; t <= i; t += 4) {
                float sc = 0.f;
                for (int d = 0; d < D; d++) sc += qs[i * DP + d] * ks[t * DP + d];
                sc *= scale;
                const float mn = fmaxf(m, sc), corr = __expf(m - mn), pw = __expf(sc - mn);
                lsum = lsum * corr + pw;
#pragma unroll
                for (int d = 0; d < 64; d++)
                    if (d < D) o[d] = o[d] * corr + pw * vs[t * DP + d];
                m = mn;
            }
        }
        // merge the 4 key lanes of a query (lanes xor 1, 2); a lane that saw no key has m = -inf, l = 0
#pragma unroll
        for (int sft = 1; sft <= 2; sft <<= 1) {
            const float om = __shfl_xor(m, sft, 64), ol = __shfl_xor(lsum, sft, 64);
            const float mn = fmaxf(m, om);
            const float c0 = m == -INFINITY ? 0.f : __expf(m - mn), c1 = om == -INFINITY ? 0.f : __expf(om - mn);
            lsum = lsum * c0 + ol * c1;
#pragma unroll
            for (int d = 0; d < 64; d++) {
                const float od = __shfl_xor(o[d], sft, 64);
                o[d] = o[d] * c0 + od * c1;
            }
            m = mn;
        }
        if (i < L) {
            float* yb = y + ((size_t)b * HD + h * D) * ld + i;
            // (static register indices: `o[d]` with d starting at the lane's kl put the 64 accumulators in scratch --
            // 272 B per thread, 0.3 GB of scratch writes per launch by PMC)
            const float inv = 1.0f / lsum;
#pragma unroll
            for (int d = 0; d < 64; d++)
                if (d < D && (d & 3) == kl) yb[(size_t)d * ld] = o[d] * inv;
        }
    }
}

int voc_launch_norm(hipStream_t s, const float* x, const float* w, const float* bias, float* y, int C, int L, int ld,
                    int kind, float eps, int B) {
    hipLaunchKernelGGL(chan_norm_kernel, dim3((unsigned)((L + 63) / 64), B), dim3(1024), 0, s, x, w, bias, y, C, L, ld, kind, eps);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

int voc_launch_attn_tile(hipStream_t s, const float* x, float* y, int H, int D, int L, int ld, int window, float theta, int B) {
    const size_t lds = (size_t)3 * L * (D + 1) * sizeof(float);
    if (D <= 0 || D > 64 || (D & 1) || L <= 0 || lds > 64 * 1024) {
        Q3_LOG("voc tile attention: head_dim %d at %d columns is not built (even, <= 64, 3 * L * (D + 1) floats <= 64 KiB)", D, L);
        return -1;
    }
    static bool attr = false;
    if (!attr) {
        Q3_HIP(hipFuncSetAttribute((const void*)voc_attn_tile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024), -1);
        attr = true;
    }
    voc_note_variant(VV_ATTN_TILE);
    hipLaunchKernelGGL(voc_attn_tile_kernel, dim3(H, B), dim3(256), lds, s, x, y, H, D, L, ld, window, theta);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

int voc_launch_attn(hipStream_t s, const float* x, float* y, int H, int D, int L, int ld, int window, float theta, int B) {
    if (D <= 0 || D > 128 || (D & 1)) {
        Q3_LOG("voc attention: head_dim %d is not built (even, <= 128)", D);
        return -1;
    }
    voc_note_variant(VV_ATTN);
    hipLaunchKernelGGL(voc_attn_kernel, dim3((unsigned)L, H, B), dim3(64), 0, s, x, y, H, D, L, ld, window, theta);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

// y[c][l] = act(x[c][l]) * x[C + c][l]; act 0 SiLU, 1 GELU
__global__ void __launch_bounds__(256) glu_kernel(const float* __restrict__ x, float* __restrict__ y, int C, int L, int ld, int act) {
    const int l = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
    if (l >= L) return;
    const float g = x[((size_t)b * 2 * C + c) * ld + l], u = x[((size_t)b * 2 * C + C + c) * ld + l];
    y[((size_t)b * C + c) * ld + l] = (act == 0 ? g / (1.0f + __expf(-g)) : gelu_erf(g)) * u;
}

int voc_launch_glu(hipStream_t s, const float* x, float* y, int C, int L, int ld, int act, int B) {
    hipLaunchKernelGGL(glu_kernel, dim3((unsigned)((L + 255) / 256), C, B), dim3(256), 0, s, x, y, C, L, ld, act);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

// Split residual VQ de-quantisation: codes i64 [B][T][NQ] -> y [B][OUT][T].
// Quantiser 0 (semantic) and 1..NQ-1 (acoustic) each sum their codebook rows ([NQ][CB][DIM]) and go
// through their own DIM->OUT projection (1x1 conv without bias); the two results add.
__global__ void __launch_bounds__(256) rvq_kernel(const int64_t* __restrict__ codes, const float* __restrict__ cb,
                                                  const float* __restrict__ p_sem, const float* __restrict__ p_ac,
                                                  float* __restrict__ y, int T, int ld, int NQ, int CB, int DIM, int OUT) {
    extern __shared__ float e[];  // [2][DIM]
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int64_t* c = codes + ((size_t)b * T + t) * 16;   // 16 ids per frame in a request (vocoder_server.py:78), the first NQ are used
    for (int d = tid; d < DIM; d += blockDim.x) {
        float s0 = 0.f, s1 = 0.f;
        const int64_t c0 = c[0];
        if (c0 >= 0 && c0 < CB) s0 = cb[((size_t)0 * CB + c0) * DIM + d];
        for (int q = 1; q < NQ; q++) {
            const int64_t cq = c[q];
            if (cq >= 0 && cq < CB) s1 += cb[((size_t)q * CB + cq) * DIM + d];
        }
        e[d] = s0;
        e[DIM + d] = s1;
    }
    __syncthreads();
    for (int o = tid; o < OUT; o += blockDim.x) {
        float acc = 0.f;
        for (int d = 0; d < DIM; d++) acc += p_sem[(size_t)o * DIM + d] * e[d];
        for (int d = 0; d < DIM; d++) acc += p_ac[(size_t)o * DIM + d] * e[DIM + d];
        y[((size_t)b * OUT + o) * ld + t] = acc;
    }
}

int voc_launch_rvq(hipStream_t s, const int64_t* codes, const float* cb, const float* p_sem, const float* p_ac, float* y, int T, int ld,
                   int NQ, int CB, int DIM, int OUT, int B) {
    hipLaunchKernelGGL(rvq_kernel, dim3(T, B), dim3(256), 2 * DIM * sizeof(float), s, codes, cb, p_sem, p_ac, y, T, ld, NQ, CB, DIM, OUT);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

// The embedding-mean front of the decoder family's Omni form (Qwen3OmniMoeCode2Wav.forward):
// y[b][c][t] = mean_q table[q * CB + codes[b][t][q]][c]; an id outside [0, CB) contributes zero.
__global__ void __launch_bounds__(256) embmean_kernel(const int64_t* __restrict__ codes, const float* __restrict__ tab,
                                                      float* __restrict__ y, int T, int ld, int NQ, int NQS, int CB, int DIM) {
    const int t = blockIdx.x, b = blockIdx.y;
    const int64_t* c = codes + ((size_t)b * T + t) * NQS;    // NQS ids per frame in the request, the first NQ are used
    for (int d = threadIdx.x; d < DIM; d += blockDim.x) {
        float s_ = 0.f;
        for (int q = 0; q < NQ; q++) {
            const int64_t cq = c[q];
            if (cq >= 0 && cq < CB) s_ += tab[((size_t)q * CB + cq) * DIM + d];
        }
        y[((size_t)b * DIM + d) * ld + t] = s_ / (float)NQ;
    }
}

int voc_launch_embmean(hipStream_t s, const int64_t* codes, const float* tab, float* y, int T, int ld, int NQ, int NQS, int CB, int DIM, int B) {
    hipLaunchKernelGGL(embmean_kernel, dim3(T, B), dim3(256), 0, s, codes, tab, y, T, ld, NQ, NQS, CB, DIM);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

// ---------------------------------------------------------------------------
// Chunk walk (voc_synthesize*, voc_synthesize_batch*): the reference assembles an utterance from its 64-frame chunks on the host
// (vocoder_server.py:84-117: first chunk kept, every next one either cross-faded over 16 frames with the tail of what
// is there, or -- shorter than the overlap -- appended).  Here the chunks of MANY utterances are decoded max_batch at a
// time and placed by two launches per batch: every chunk copies its samples behind the blended head to its position,
// then every blended chunk folds its head into the 30 720 samples already there (written by its predecessor's copy,
// this batch or an earlier one).  A chunk shorter than twice the overlap has no successor (the walk steps by
// chunk - 16 frames), so no sample is blended twice and the two-pass order reproduces the sequential result bit for bit:
// float32 products and one float32 add, never fused (numpy: result[-OV:] * fade_out + chunk[:OV] * fade_in), the fade
// np.linspace(1, 0, OV, dtype=float32) evaluated in double exactly as numpy does.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) voc_place_copy_kernel(const float* __restrict__ dec, int pitch, const ChunkPlace* __restrict__ pl,
                                                             float* __restrict__ out) {
    const ChunkPlace p = pl[blockIdx.y];
    const float* src = dec + (size_t)p.row * pitch;
    for (int i = p.head + blockIdx.x * 256 + threadIdx.x; i < p.len; i += gridDim.x * 256) out[p.dst + i] = src[i];
}

__global__ void __launch_bounds__(256) voc_place_blend_kernel(const float* __restrict__ dec, int pitch, const ChunkPlace* __restrict__ pl,
                                                              float* __restrict__ out, int OV) {
    const ChunkPlace p = pl[blockIdx.y];
    if (p.head == 0) return;
    const float* src = dec + (size_t)p.row * pitch;
    const double step = -1.0 / (double)(OV - 1);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < OV; i += gridDim.x * 256) {
        const float fo = (i == OV - 1) ? 0.0f : (float)(1.0 + (double)i * step);
        const float fi = __fsub_rn(1.0f, fo);
        out[p.dst + i] = __fadd_rn(__fmul_rn(out[p.dst + i], fo), __fmul_rn(src[i], fi));
    }
}

int voc_launch_place(hipStream_t s, const float* dec, int pitch, const ChunkPlace* pl, float* out, int OV, int B) {
    hipLaunchKernelGGL(voc_place_copy_kernel, dim3(64, B), dim3(256), 0, s, dec, pitch, pl, out);
    hipLaunchKernelGGL(voc_place_blend_kernel, dim3(32, B), dim3(256), 0, s, dec, pitch, pl, out, OV);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

// np.clip(audio * 32767, -32768, 32767).astype(np.int16) (vocoder_server.py:175): float32 product, truncation toward zero
__device__ __forceinline__ int16_t voc_int16(float x) {
    float v = __fmul_rn(x, 32767.0f);
    v = v < -32768.0f ? -32768.0f : (v > 32767.0f ? 32767.0f : v);
    return (int16_t)v;
}
__device__ __forceinline__ void voc_store(float* y, long long i, float x) { y[i] = x; }
__device__ __forceinline__ void voc_store(int16_t* y, long long i, float x) { y[i] = voc_int16(x); }

__global__ void __launch_bounds__(256) voc_to_int16_kernel(const float* __restrict__ x, int16_t* __restrict__ y, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    y[i] = voc_int16(x[i]);
}

int voc_launch_to_int16(hipStream_t s, const float* x, int16_t* y, long long n) {
    hipLaunchKernelGGL(voc_to_int16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, y, n);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

// ---------------------------------------------------------------------------
// Streaming chunk walk (voc_stream_*): between pushes each stream keeps only the last OV assembled samples -- the ones the
// next chunk's cross-fade may still change -- in its slot of `tail` ([max_streams][OV] on the device).  A push lays every
// stream it touches out as one window of its work buffer: the kept tail first (load), then the chunks the push decodes,
// placed by voc_place_copy/blend at window coordinates; emit hands [0, n_out) of the window to the caller's packed output
// (f32, or the int16 rule) and keeps [n_out, n_out + tail_out) as the stream's new tail.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) voc_stream_load_kernel(const float* __restrict__ tail, int OV, const StreamWin* __restrict__ w,
                                                              float* __restrict__ work) {
    const StreamWin p = w[blockIdx.y];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < p.tail_in; i += gridDim.x * 256) work[p.win + i] = tail[(size_t)p.stream * OV + i];
}

template <typename T>
__global__ void __launch_bounds__(256) voc_stream_emit_kernel(const float* __restrict__ work, const StreamWin* __restrict__ w,
                                                              float* __restrict__ tail, int OV, T* __restrict__ out) {
    const StreamWin p = w[blockIdx.y];
    for (long long i = blockIdx.x * 256 + threadIdx.x; i < p.n_out; i += gridDim.x * 256) voc_store(out, p.out + i, work[p.win + i]);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < p.tail_out; i += gridDim.x * 256)
        tail[(size_t)p.stream * OV + i] = work[p.win + p.n_out + i];
}

int voc_launch_stream_load(hipStream_t s, const float* tail, int OV, const StreamWin* w, float* work, int n) {
    hipLaunchKernelGGL(voc_stream_load_kernel, dim3(64, n), dim3(256), 0, s, tail, OV, w, work);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

int voc_launch_stream_emit(hipStream_t s, const float* work, const StreamWin* w, float* tail, int OV, void* out, bool want16, int n) {
    if (want16) hipLaunchKernelGGL(voc_stream_emit_kernel<int16_t>, dim3(64, n), dim3(256), 0, s, work, w, tail, OV, (int16_t*)out);
    else hipLaunchKernelGGL(voc_stream_emit_kernel<float>, dim3(64, n), dim3(256), 0, s, work, w, tail, OV, (float*)out);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

// ---------------------------------------------------------------------------
// Carry-state incremental decode (voc_incr_*): every op with a receptive field keeps, per stream, the last H columns of its
// input ([max_streams][C][H] on the device, zero at the start of a stream = the causal padding the kernels assume).  A push
// lays [history | new columns] out in the work buffer, runs the op's ordinary kernel over it and drops the history's outputs.
// ---------------------------------------------------------------------------
// Columns [skip, skip + n) of channels [c0, c0 + C) of src ([B][src_C][src_ld]) -> dst [B][C][dst_ld] behind the H history
// columns of the entry's stream; the last H columns of [history | new] become the stream's new history.  One workgroup
// (blockIdx.x == 0) owns a row's history: it reads all of it before it writes any (H <= 256, the launcher's rule).
// parity (null: the history lives in hist0 and moves on in place): entry b reads hist{parity[b]} and writes the other buffer,
// so that a push can be dropped per entry (the split arithmetic's redo).
__global__ void __launch_bounds__(256) voc_incr_prepend_kernel(const float* __restrict__ src, int src_C, int c0, int src_ld, int skip,
                                                               float* __restrict__ dst, int C, int dst_ld, float* hist0, float* hist1,
                                                               const int* __restrict__ parity, int H, int n, long long state_floats,
                                                               const int* __restrict__ streams) {
    const int c = blockIdx.y, b = blockIdx.z;
    const float* s = src + ((size_t)b * src_C + c0 + c) * src_ld + skip;
    float* d = dst + ((size_t)b * C + c) * dst_ld;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) d[H + j] = s[j];
    if (blockIdx.x == 0 && H > 0) {
        const size_t ho = (size_t)streams[b] * state_floats + (size_t)c * H;
        const int par = parity ? parity[b] : 0;
        const float* h = (par ? hist1 : hist0) + ho;
        float* hw = (parity ? (par ? hist0 : hist1) : hist0) + ho;
        const int i = threadIdx.x;
        float old = 0.f, nw = 0.f;
        if (i < H) {
            old = h[i];
            nw = (i + n < H) ? h[i + n] : s[i + n - H];
        }
        __syncthreads();
        if (i < H) {
            d[i] = old;
            hw[i] = nw;
        }
    }
}

int voc_launch_incr_prepend(hipStream_t s, const float* src, int src_C, int c0, int src_ld, int skip, float* dst, int C, int dst_ld,
                            float* hist0, float* hist1, const int* parity, int H, int n, long long state_floats, const int* streams, int B) {
    hipLaunchKernelGGL(voc_incr_prepend_kernel, dim3((unsigned)std::min(64, (n + 255) / 256), C, B), dim3(256), 0, s, src, src_C, c0, src_ld,
                       skip, dst, C, dst_ld, hist0, hist1, parity, H, n, state_floats, streams);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

// The same assembly for a conv that runs on the split-precision path: columns [skip, skip + n) of src ([B][C][src_ld]) join the H
// history columns of the entry's stream, and [history | new] (L = H + n columns) goes out as the consuming conv's input planes --
// its Snake / GELU applied, {hi, lo} fp16 [B][C/8][L][8], split as snake_split_kernel splits -- and, where dst is given (the
// consumer saves a residual: the residual IS this buffer), as f32 [B][C][dst_ld].  The history itself stays f32 (the planes are
// a pure function of it, rebuilt every push; Snake(0) = GELU(0) = 0 keeps the causal zero padding valid) and always moves from
// hist{parity[b]} to the other buffer, so no thread reads what another writes and H is not bounded by a workgroup.
// snake_split_kernel's access pattern: lanes run along the columns (each row read is a run of consecutive floats), a lane owns the
// 8 channels of one column and stores one 16-byte record per plane.  ovf[b] = 1 when a plane value of entry b leaves +-65504
// or is a NaN.
__global__ void __launch_bounds__(256) voc_incr_prepend_split_kernel(const float* __restrict__ src, int src_ld, int skip,
                                                                     _Float16* __restrict__ xh, _Float16* __restrict__ xl,
                                                                     float* __restrict__ dst, int dst_ld, int C,
                                                                     const float* __restrict__ alpha, const float* __restrict__ inv_beta,
                                                                     int gelu, float* hist0, float* hist1,
                                                                     const int* __restrict__ parity, int H, int n, long long state_floats,
                                                                     const int* __restrict__ streams, int* __restrict__ ovf) {
    const int l = blockIdx.x * 256 + threadIdx.x, cg = blockIdx.y, b = blockIdx.z;   // cg: 8-channel group
    const int L = H + n;
    if (l >= L) return;
    const size_t ho = (size_t)streams[b] * state_floats + (size_t)cg * 8 * H;
    const int par = parity[b];
    const float* hr = (par ? hist1 : hist0) + ho;
    float* hw = (par ? hist0 : hist1) + ho;
    const float* sp = src + ((size_t)b * C + cg * 8) * src_ld + skip;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = l < H ? hr[(size_t)j * H + l] : sp[(size_t)j * src_ld + (l - H)];
    if (l >= n) {   // the last H columns of [history | new] are the stream's next history
#pragma unroll
        for (int j = 0; j < 8; j++) hw[(size_t)j * H + (l - n)] = v[j];
    }
    if (dst) {
        float* dp = dst + ((size_t)b * C + cg * 8) * dst_ld + l;
#pragma unroll
        for (int j = 0; j < 8; j++) dp[(size_t)j * dst_ld] = v[j];
    }
    if (alpha) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float sn = __sinf(alpha[cg * 8 + j] * v[j]);
            v[j] = v[j] + inv_beta[cg * 8 + j] * (sn * sn);
        }
    }
    if (gelu) {
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = gelu_erf(v[j]);
    }
    hv8 h, lo;
    bool big = false;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        big |= !(fabsf(v[j]) <= 65504.f);
        const _Float16 hi = (_Float16)fminf(fmaxf(v[j], -65504.f), 65504.f);
        h[j] = hi;
        lo[j] = (_Float16)((v[j] - (float)hi) * 2048.0f);
    }
    const size_t o = (((size_t)b * (C >> 3) + cg) * L + l) * 8;
    *(hv8*)(xh + o) = h;
    *(hv8*)(xl + o) = lo;
    if (big) ovf[b] = 1;
}

int voc_launch_incr_prepend_split(hipStream_t s, const float* src, int src_ld, int skip, _Float16* xh, _Float16* xl, float* dst, int dst_ld,
                                  int C, const float* alpha, const float* inv_beta, int gelu, float* hist0, float* hist1, const int* parity,
                                  int H, int n, long long state_floats, const int* streams, int* ovf, int B) {
    if (C % 8 || H <= 0 || n <= 0 || !hist1 || !parity || !ovf) return -1;
    hipLaunchKernelGGL(voc_incr_prepend_split_kernel, dim3((unsigned)((H + n + 255) / 256), C / 8, B), dim3(256), 0, s, src, src_ld, skip, xh,
                       xl, dst, dst_ld, C, alpha, inv_beta, gelu, hist0, hist1, parity, H, n, state_floats, streams, ovf);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

// voc_attn_kernel for the incremental decode: queries are the n new columns of x ([B][3*H*D][x_ld], at column skip + i), keys
// and values come from kv = [carried window | new] ([B][2*H*D][kv_ld], k rows then v rows, new column i at Hk + i), and the
// window is placed by the ABSOLUTE column pos0[b] + i of the stream.  RoPE scores depend on the distance of query and key only:
// both are rotated by their offset from the first key of the query's window (= their absolute column while the stream is
// shorter than the window), so the angles stay below `window` and their rounding does not grow with the stream's length.
// One wave per (query, head) walks its keys in order, so a column's bits depend on nothing but its own window: not on the
// push it arrives in, nor on the batch.  No LDS: the [window - 1 + n] columns of a head (up to 135 x 64 x 2 floats) come from L2.
__global__ void __launch_bounds__(64) voc_attn_incr_kernel(const float* __restrict__ x, int x_ld, int skip, const float* __restrict__ kv,
                                                           int kv_ld, int Hk, float* __restrict__ y, int H, int D, int window,
                                                           float theta, const int* __restrict__ pos0) {
    const int i = blockIdx.x, h = blockIdx.y, b = blockIdx.z, j = threadIdx.x;
    const int half = D / 2, HD = H * D;
    const bool on = j < half;
    const int p0 = pos0[b], pos = p0 + i;
    const float inv_freq = on ? __powf(theta, -2.0f * (float)j / (float)D) : 0.f;
    auto rope = [&](const float* base, int ld, int col, int at, float& a, float& c) {   // rows (j, j+half) of a head
        float x0 = 0.f, x1 = 0.f;
        if (on) {
            x0 = base[(size_t)j * ld + col];
            x1 = base[(size_t)(j + half) * ld + col];
        }
        float sn, cs;
        __sincosf((float)at * inv_freq, &sn, &cs);
        a = x0 * cs - x1 * sn;
        c = x1 * cs + x0 * sn;
    };
    const int t0 = pos - window + 1 > 0 ? pos - window + 1 : 0;
    float q0, q1;
    rope(x + ((size_t)b * 3 * HD + h * D) * x_ld, x_ld, skip + i, pos - t0, q0, q1);
    const float* kb = kv + ((size_t)b * 2 * HD + h * D) * kv_ld;
    const float* vb = kb + (size_t)HD * kv_ld;
    const float scale = 1.0f / sqrtf((float)D);
    float m = -INFINITY, lsum = 0.f, o0 = 0.f, o1 = 0.f;
    for (int t = t0; t <= pos; t++) {
        const int col = Hk + (t - p0);       // >= 0: t >= pos - (window - 1) >= p0 - Hk
        float k0, k1;
        rope(kb, kv_ld, col, t - t0, k0, k1);
        float sc = q0 * k0 + q1 * k1;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sc += __shfl_xor(sc, o, 64);
        sc *= scale;
        const float mn = fmaxf(m, sc), corr = __expf(m - mn), p = __expf(sc - mn);
        float v0 = 0.f, v1 = 0.f;
        if (on) {
            v0 = vb[(size_t)j * kv_ld + col];
            v1 = vb[(size_t)(j + half) * kv_ld + col];
        }
        lsum = lsum * corr + p;
        o0 = o0 * corr + p * v0;
        o1 = o1 * corr + p * v1;
        m = mn;
    }
    if (on) {
        float* yb = y + ((size_t)b * HD + h * D) * x_ld + skip + i;
        yb[(size_t)j * x_ld] = o0 / lsum;
        yb[(size_t)(j + half) * x_ld] = o1 / lsum;
    }
}

int voc_launch_incr_attn(hipStream_t s, const float* x, int x_ld, int skip, const float* kv, int kv_ld, int Hk, float* y, int H, int D,
                         int window, float theta, const int* pos0, int n, int B) {
    hipLaunchKernelGGL(voc_attn_incr_kernel, dim3((unsigned)n, H, B), dim3(64), 0, s, x, x_ld, skip, kv, kv_ld, Hk, y, H, D, window, theta, pos0);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

// the n samples of every entry (row b of y, from column skip) -> the caller's packed output (f32, or the int16 rule)
template <typename T>
__global__ void __launch_bounds__(256) voc_incr_emit_kernel(const float* __restrict__ y, int ld, int skip, int n,
                                                            const long long* __restrict__ out_off, T* __restrict__ out) {
    const int b = blockIdx.y;
    const long long o = out_off[b];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) voc_store(out, o + i, y[(size_t)b * ld + skip + i]);
}

int voc_launch_incr_emit(hipStream_t s, const float* y, int ld, int skip, int n, const long long* out_off, void* out, bool want16, int B) {
    const dim3 grid((unsigned)std::min(64, (n + 255) / 256), B);
    if (want16) hipLaunchKernelGGL(voc_incr_emit_kernel<int16_t>, grid, dim3(256), 0, s, y, ld, skip, n, out_off, (int16_t*)out);
    else hipLaunchKernelGGL(voc_incr_emit_kernel<float>, grid, dim3(256), 0, s, y, ld, skip, n, out_off, (float*)out);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

// Snapshots of a stream's carried state (voc_incr_restore): entry blockIdx.y copies `floats` floats from its slot into its
// stream's history -- into both history buffers where the object is double-buffered (dst1 != null), so that an op the next push
// does not reach finds the same columns whichever buffer it reads.  16 bytes per lane over the whole float4 groups, grid-strided;
// the floats behind the last whole group go one per lane (workgroup 0 of the entry).  A stream's state starts at stream *
// floats: with 4 | floats (the default table) every entry is 16-byte aligned; an entry that is not takes the scalar loop whole.
__global__ void __launch_bounds__(256) voc_incr_restore_kernel(const SnapCopy* __restrict__ tab, long long floats) {
    const SnapCopy e = tab[blockIdx.y];
    const long long first = (long long)blockIdx.x * 256 + threadIdx.x, step = (long long)gridDim.x * 256;
    if ((((uintptr_t)e.src | (uintptr_t)e.dst0 | (uintptr_t)e.dst1) & 15) != 0) {
        for (long long i = first; i < floats; i += step) {
            const float x = e.src[i];
            e.dst0[i] = x;
            if (e.dst1) e.dst1[i] = x;
        }
        return;
    }
    const long long nvec = floats / 4;
    const float4* __restrict__ s4 = (const float4*)e.src;
    float4* d0 = (float4*)e.dst0;
    float4* d1 = (float4*)e.dst1;
    for (long long i = first; i < nvec; i += step) {
        const float4 x = s4[i];
        d0[i] = x;
        if (d1) d1[i] = x;
    }
    const long long t = nvec * 4 + threadIdx.x;
    if (blockIdx.x == 0 && t < floats) {
        const float x = e.src[t];
        e.dst0[t] = x;
        if (e.dst1) e.dst1[t] = x;
    }
}

// The grid follows the bytes: one workgroup per 256 float4 groups of an entry, capped so that the n entries together stay
// near 2048 workgroups (8 per compute unit); the kernel strides over the rest.
int voc_launch_incr_restore(hipStream_t s, const SnapCopy* tab, long long floats, int n) {
    if (n <= 0) return 0;
    if (n > 65535) {   // (gridDim.y; an object of that many streams does not fit a device)
        Q3_LOG("voc_incr_restore: %d entries in one call", n);
        return -1;
    }
    const long long want = std::max(1LL, (floats / 4 + 255) / 256), cap = std::max(1, 2048 / n);
    hipLaunchKernelGGL(voc_incr_restore_kernel, dim3((unsigned)std::min(want, cap), (unsigned)n), dim3(256), 0, s, tab, floats);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

}  // namespace q3

using namespace q3;

extern "C" {

int voc_set_narrow_k1(int on) {   // test hook: 128-column tiles for the 1-tap convs (default on)
    voc_settings.set_narrow_k1(on);
    return 0;
}

// test hook: the workgroup target below which launch_conv_mt takes shorter tiles and launch_conv_split 64-row ones (512, or
// Q3_VOC_FILL for the exact path).  n >= 0 replaces it for the process (0: tile height follows divisibility alone), n < 0
// restores the default.  -> the value set.
int voc_set_fill(int n) {
    return voc_settings.set_fill(n);
}

// test hook: the instantiation the last conv launch of the calling thread took ("conv<4,1,16,ct0,act1>", "out1", "resunit<3>",
// "split<7,1,3,1>/myfast", "snake_split", or "snake_split+split<...>" for a split conv that read the separate pass's planes;
// "attn_tile" / "attn" after a full-chunk attention launch; "" before the first one)
const char* voc_debug_last_variant() {
    static thread_local char name[64];
    const int* p = voc_variant.p;
    switch (voc_variant.kind) {
        case VV_CONV: snprintf(name, sizeof(name), "conv<%d,%d,%d,ct%d,act%d>", p[0], p[1], p[2], p[3], p[4]); break;
        case VV_OUT1: snprintf(name, sizeof(name), "out1"); break;
        case VV_RESUNIT: snprintf(name, sizeof(name), "resunit<%d>", p[0]); break;
        case VV_SNAKE_SPLIT: snprintf(name, sizeof(name), "snake_split"); break;
        case VV_ATTN_TILE: snprintf(name, sizeof(name), "attn_tile"); break;
        case VV_ATTN: snprintf(name, sizeof(name), "attn"); break;
        case VV_SPLIT:
            snprintf(name, sizeof(name), "%ssplit<%d,%d,%d,%d>%s", voc_variant.after_pass ? "snake_split+" : "", p[0], p[1], p[2], p[3],
                     p[4] ? "/myfast" : "");
            break;
        default: name[0] = 0;
    }
    return name;
}

// Cap the number of workgroups every vocoder launch may occupy (0 = no cap).  Process-wide.
int voc_set_max_workgroups(int n) {   // -> the cap in effect (0 = none)
    if (n < 0) {   // one persistent workgroup per compute unit: the co-run setting (qwen3tts_voc.h)
        int dev = 0;
        hipDeviceProp_t p;
        n = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess) ? p.multiProcessorCount : 0;
    }
    return voc_settings.set_max_workgroups(n);
}

}  // extern "C"
