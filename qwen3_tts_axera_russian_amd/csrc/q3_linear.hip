// q3_linear.hip -- gfx950 (MI355X, CDNA4) linear layers of the Qwen3-TTS talker / code-predictor decode path and of
// the prefill.  Wave = 64 lanes everywhere.
//
// Hot-path map (reference file:line each kernel stands in for):
//   linear_kernel   every projection llama_decode / the ONNX decode step runs
//                   (llama_wrapper.c:145, code_predictor_server.py:80), as a
//                   weight-streaming MFMA 16x16x32 f16 kernel with split-K over
//                   the waves of a workgroup; RMSNorm fused as prologue, residual
//                   add / SwiGLU fused as epilogue.
//   gemm_kernel / gemm_glds_kernel   the same layers for many rows (prefill), as tiled GEMMs.
#include "q3_kdev.h"

namespace q3 {

// ---------------------------------------------------------------------------
// Weight repack: row-major [N][K] fp16 -> fragment order.  Element (n,k) goes
// to ((t*KB + kb)*64 + lane)*8 + j with t=n/16, kb=k/32, lane=(n%16)+16*((k%32)/8),
// j=k%8: one 16x32 weight block is one 1 KiB wave-wide 16-B-per-lane load whose
// lane contents are exactly the B operand of v_mfma_f32_16x16x32_f16.
// ---------------------------------------------------------------------------
__global__ void pack_linear_kernel(const half_t* __restrict__ src, int N, int K, half_t* __restrict__ dst,
                                   int tile_off, int tile_stride) {
    const int KB = K / 32;
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // one 16-B group each
    size_t total = (size_t)(N / 16) * KB * 64;
    if (idx >= total) return;
    int lane = (int)(idx & 63);
    size_t blk = idx >> 6;
    int kb = (int)(blk % KB);
    int ts = (int)(blk / KB);
    int n = ts * 16 + (lane & 15);
    int k = kb * 32 + (lane >> 4) * 8;
    h8 v = *(const h8*)(src + (size_t)n * K + k);
    size_t td = (size_t)tile_off + (size_t)ts * tile_stride;
    *(h8*)(dst + ((td * KB + kb) * 64 + lane) * 8) = v;
}

int launch_pack_linear(hipStream_t s, const half_t* src, int N, int K, half_t* dst, int tile_off,
                       int tile_stride) {
    if (N % 16 || K % 32) {
        Q3_LOG("pack_linear: N=%d K=%d not multiples of 16/32", N, K);
        return -1;
    }
    size_t total = (size_t)(N / 16) * (K / 32) * 64;
    int blocks = (int)((total + 255) / 256);
    hipLaunchKernelGGL(pack_linear_kernel, dim3(blocks), dim3(256), 0, s, src, N, K, dst, tile_off, tile_stride);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

// Which instantiation the last launch_linear call picked ("" when it launched nothing): the kernel-level tests assert
// the dispatch instead of guessing it.  Every launcher below formats its name once and stores the pointer per launch.
static const char* g_last_variant = "";
const char* last_linear_variant() { return g_last_variant; }
static const char* pro_name(int pro) { return pro == PRO_NORM ? "NORM" : "F16"; }
static const char* epi_name(int epi) { return epi == EPI_STORE ? "STORE" : epi == EPI_RESID ? "RESID" : "SWIGLU"; }
static int env_int(const char* name, int dflt) { return getenv(name) ? atoi(getenv(name)) : dflt; }

// ---------------------------------------------------------------------------
// linear_kernel<NB16, MT16, KBW, NW, PRO, EPI, NT>
//   workgroup = NW waves; it owns NB16 column tiles (16 weight rows each) for
//   MT16*16 batch rows; wave w owns k-blocks [w*KBW, (w+1)*KBW) (32 k each), so
//   K = NW*KBW*32.  All of a wave's weight fragments are requested up front
//   (KBW*NB16 16-B loads per lane in flight: the HBM stream), the A fragments
//   come from L2, partial tiles are summed across waves through LDS in a fixed
//   order (deterministic), then the epilogue runs on the summed tile.
// ---------------------------------------------------------------------------
// The first arguments are the ones the load addresses need: with -amdgpu-kernarg-preload-count=16 they
// arrive in SGPRs at wave launch instead of behind two dependent scalar-memory round trips.
template <int NB16, int MT16, int KBW, int NW, int PRO, int EPI, bool NT>
__global__ void __launch_bounds__(NW * 64)
    linear_kernel(const half_t* __restrict__ p_wp, const void* __restrict__ p_asrc, const float* __restrict__ p_ssq,
                  const float* __restrict__ p_gamma, void* __restrict__ p_out, int p_M, int p_N, int p_m_begin,
                  int p_swap, float p_eps, LinArgs a) {
    a.wp = p_wp;
    a.x16 = (const half_t*)p_asrc;
    a.ssq = p_ssq;
    a.gamma = p_gamma;
    a.y = (float*)p_out;
    a.h_out = (float*)p_out;
    a.act = (half_t*)p_out;
    a.M = p_M;
    a.N = p_N;
    a.m_begin = p_m_begin;
    a.swap_grid = p_swap;
    a.eps = p_eps;
    constexpr int MR = MT16 * 16, NB = NB16 * 16, NBP = NB + 4, KB = NW * KBW, K = KB * 32;
    constexpr int NTH = NW * 64;
    constexpr int NOUT = (EPI == EPI_SWIGLU) ? MR * NB / 2 : MR * NB;   // outputs of this workgroup
    constexpr int OPT = (NOUT + NTH - 1) / NTH;                         // outputs per thread
    constexpr int SQI = (MR * 16 + NTH - 1) / NTH;                      // ssq float4 groups per thread
    Q3_TL(10 + PRO * 4 + EPI);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int q = lane >> 4, c = lane & 15;
    // many row blocks (prefill): the row block is the fast grid index, so the blocks that share a
    // weight tile run back to back and the tile is streamed from HBM once
    const int tile0 = (a.swap_grid ? blockIdx.y : blockIdx.x) * NB16;
    const int m0 = a.m_begin + (a.swap_grid ? blockIdx.x : blockIdx.y) * MR;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* red = (float*)smem;             // [NW][MR][NBP]
    float* inv_s = red + NW * MR * NBP;    // [MR]

    // ---- 1. every global load of the kernel is issued here: nothing later starts a second memory
    // round trip.  vmcnt retires in order, so the few operands that gate the prologue go first, the
    // HBM weight stream next, and the L2-resident fragments (needed only together with the weights) last.
    float4 sq[SQI];
    h8 af[MT16][KBW];
    float hold[OPT], gnext[OPT];
    // (a) tiny operands that gate the prologue / epilogue
    if (PRO == PRO_NORM) {
#pragma unroll
        for (int i = 0; i < SQI; i++) {
            // float4 group: row = g4/16 (64 partials = 16 float4).  UNCONDITIONAL load (index clamped; rows beyond a.M are
            // allocated padding of the row block): a predicated load becomes a branch, and the compiler sinks the first
            // use of the loaded value -- with its s_waitcnt vmcnt(0) -- into that branch, ahead of the weight stream's
            // issue: a whole dependent memory round trip in front of every normed GEMM (seen in the ISA, round 2)
            const int g4 = tid + i * NTH, g4c = g4 < MR * 16 ? g4 : 0;
            sq[i] = *(const float4*)(a.ssq + (size_t)(m0 + g4c / 16) * 64 + (g4c & 15) * 4);
        }
    }
    if (EPI == EPI_RESID) {
#pragma unroll
        for (int i = 0; i < OPT; i++) {
            const int o = tid + i * NTH;
            const int m = m0 + o / NB;
            hold[i] = 0.f;
            gnext[i] = 0.f;
            if (o < NOUT && m < a.M) hold[i] = a.h_out[frag_idx(m, tile0 * 16 + (o % NB), a.N)];
            if (o < NOUT && a.gamma) gnext[i] = a.gamma[tile0 * 16 + (o % NB)];   // the consumer's norm weight
        }
    }
    // (b) / (c): the weight stream (HBM, the long pole: everything this wave will need, in flight at once) and the
    // activation fragments (L2; fp16 in either prologue -- PRO_NORM reads the producer's pre-scaled xh).
    h8 wf[NB16][KBW];
#pragma unroll
    for (int nb = 0; nb < NB16; nb++)
#pragma unroll
        for (int kbi = 0; kbi < KBW; kbi++) {
            const h8* p = (const h8*)(a.wp + (((size_t)(tile0 + nb) * KB + (size_t)w * KBW + kbi) * 64 + lane) * 8);
            wf[nb][kbi] = NT ? __builtin_nontemporal_load(p) : *p;
        }
#pragma unroll
    for (int kbi = 0; kbi < KBW; kbi++) {
        const int k0 = (w * KBW + kbi) * 32 + q * 8;
#pragma unroll
        for (int mt = 0; mt < MT16; mt++) {
            // rows beyond a.M are padding of the last 16-row block (allocated, never stored from)
            af[mt][kbi] = *(const h8*)(a.x16 + frag_idx(m0 + mt * 16 + c, k0, K));
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    // the epilogue's scalar arguments beyond the preloaded ones: fetched now, under the weight stream, not at the epilogue
    if (EPI == EPI_RESID) Q3_FETCH_ARGS("s"(a.ssq_out), "s"(a.xh_out));
    if (EPI == EPI_STORE) Q3_FETCH_ARGS("s"(a.ldy));
    if (PRO == PRO_NORM) Q3_FETCH_ARGS("s"(a.eps));
    Q3_PH(0);  // all loads issued

    // ---- 2. RMSNorm scale per row from the producer's 64 sum-of-squares partials (a.ssq_parts == 64): only the
    // epilogue needs it (the LDS reduction's barrier orders it) ----
    if (PRO == PRO_NORM) {
#pragma unroll
        for (int i = 0; i < SQI; i++) {
            const int g4 = tid + i * NTH;
            float s = (sq[i].x + sq[i].y) + (sq[i].z + sq[i].w);
            s = group_sum_down<16>(s);
            if (g4 < MR * 16 && (g4 & 15) == 0) inv_s[g4 / 16] = (1.0f / sqrtf(s / (float)K + a.eps)) * NORM_POST;
        }
    }

    Q3_PH(1);  // prologue done (norm scale known, activations converted)
    // ---- 3. MFMA over this wave's K slice ----
    f4 acc[MT16][NB16];
#pragma unroll
    for (int mt = 0; mt < MT16; mt++)
#pragma unroll
        for (int nb = 0; nb < NB16; nb++) acc[mt][nb] = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kbi = 0; kbi < KBW; kbi++)
#pragma unroll
        for (int mt = 0; mt < MT16; mt++)
#pragma unroll
            for (int nb = 0; nb < NB16; nb++)
                acc[mt][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[mt][kbi], wf[nb][kbi], acc[mt][nb], 0, 0, 0);

    asm volatile("" ::"v"(acc[0][0][0]));  // (diagnostic stamp below must not float above the MFMAs)
    Q3_PH(2);  // MFMAs done (weights landed)
    // ---- 4. partial tiles -> LDS.  D layout: col = lane&15, row = 4*(lane>>4) + reg.  (A layout with the four
    // accumulator registers of a lane adjacent -- one ds_write_b128 per tile instead of four scalar stores -- was
    // measured in round 3: 2.420 against 2.410 ms per frame at 32 rows, no gain.) ----
#define RED(w_, row_, col_) red[((w_) * MR + (row_)) * NBP + (col_)]
#pragma unroll
    for (int mt = 0; mt < MT16; mt++)
#pragma unroll
        for (int nb = 0; nb < NB16; nb++)
#pragma unroll
            for (int r = 0; r < 4; r++) RED(w, mt * 16 + 4 * q + r, nb * 16 + c) = acc[mt][nb][r];
    __syncthreads();
    Q3_PH(3);  // partials in LDS, barrier passed

    // ---- 5. fixed-order sum over waves + epilogue ----
    if (EPI == EPI_STORE || EPI == EPI_RESID) {
#pragma unroll
        for (int i = 0; i < OPT; i++) {
            const int o = tid + i * NTH;
            if (o < NOUT) {   // wave-uniform (NOUT and NTH are multiples of 64)
                const int mr = o / NB, n = o % NB;
                float v = 0.f;
#pragma unroll
                for (int ww = 0; ww < NW; ww++) v += RED(ww, mr, n);
                const int m = m0 + mr;
                const int ng = tile0 * 16 + n;
                const bool ok = m < a.M;
                if (PRO == PRO_NORM) v *= inv_s[mr];
                if (EPI == EPI_STORE) {
                    if (ok) Q3_OUT_STORE(v, &a.y[(size_t)m * a.ldy + ng]);
                } else {
                    const float hn = ok ? hold[i] + v : 0.f;
                    if (ok) Q3_OUT_STORE(hn, &a.h_out[frag_idx(m, ng, a.N)]);
                    if (ok && a.xh_out) Q3_OUT_STORE(pre_scaled(hn, gnext[i]), &a.xh_out[frag_idx(m, ng, a.N)]);
                    const float s = group_sum_down<16>(hn * hn);
                    if (ok && (n & 15) == 0) Q3_OUT_STORE(s, &a.ssq_out[(size_t)m * (a.N / 16) + (ng >> 4)]);
                }
            }
        }
    } else {  // EPI_SWIGLU: tile 2i = gate rows, tile 2i+1 = the matching up rows
        constexpr int NH = NB / 2;
#pragma unroll
        for (int i = 0; i < OPT; i++) {
            const int o = tid + i * NTH;
            if (o < NOUT) {
                const int mr = o / NH, j = o % NH;
                const int ii = j >> 4, cc = j & 15;
                float g = 0.f, u = 0.f;
#pragma unroll
                for (int ww = 0; ww < NW; ww++) {
                    g += RED(ww, mr, (2 * ii) * 16 + cc);
                    u += RED(ww, mr, (2 * ii + 1) * 16 + cc);
                }
                const int m = m0 + mr;
                if (PRO == PRO_NORM) {
                    g *= inv_s[mr];
                    u *= inv_s[mr];
                }
                if (m < a.M) {
                    const float sg = __fdividef(g, 1.0f + __expf(-g));   // hardware exp/rcp: ~1e-6 relative, far below the fp16 rounding that follows
                    Q3_OUT_STORE(sat_half(sg * u), &a.act[frag_idx(m, (tile0 / NB16) * NH + j, a.N / 2)]);
                }
            }
        }
    }
#undef RED
}

template <int NB16, int MT16, int KBW, int NW, int PRO, int EPI, bool NT>
static int launch_linear_nt(hipStream_t s, const LinArgs& a) {
    constexpr int MR = MT16 * 16, NBP = NB16 * 16 + 4;
    constexpr size_t lds = (size_t)NW * MR * NBP * 4 + MR * 4;
    static bool attr_set = false;
    if (!attr_set) {
        if (lds > 48 * 1024)
            Q3_HIP(hipFuncSetAttribute((const void*)linear_kernel<NB16, MT16, KBW, NW, PRO, EPI, NT>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), -1);
        attr_set = true;
    }
    static char name[64];
    if (!name[0])
        snprintf(name, sizeof(name), "linear<%d,%d,%d,%d,%s,%s,%s>", NB16, MT16, KBW, NW, pro_name(PRO), epi_name(EPI), NT ? "nt" : "t");
    g_last_variant = name;
    LinArgs b = a;
    b.tl_node = tl_next_node();
    const unsigned nt_ = a.N / (16 * NB16), nr_ = (a.M - a.m_begin + MR - 1) / MR;
    b.swap_grid = nr_ > 2 ? 1 : 0;
    dim3 grid(b.swap_grid ? nr_ : nt_, b.swap_grid ? nt_ : nr_);
    const void* asrc = (const void*)b.x16;
    void* outp = EPI == EPI_STORE ? (void*)b.y : EPI == EPI_RESID ? (void*)b.h_out : (void*)b.act;
    hipLaunchKernelGGL((linear_kernel<NB16, MT16, KBW, NW, PRO, EPI, NT>), grid, dim3(NW * 64), lds, s, b.wp, asrc, b.ssq,
                       b.gamma, outp, b.M, b.N, b.m_begin, b.swap_grid, b.eps, b);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

// Tile of a workgroup in the tiled GEMMs.  Workgroups are dealt to the 8 XCDs round-robin (linear id % 8), and every
// XCD has its own L2: the R row tiles that share one weight column tile must sit on ONE XCD, or that tile is pulled
// from HBM / Infinity Cache eight times (measured: the 971-row q/k/v GEMM moved ~80 MB for 8.4 MB of weights).
// XCD x therefore owns column tiles x, x + 8, ...; its j-th workgroup is (row tile j % R, column tile x + 8 * (j / R)).
__device__ __forceinline__ void gemm_tile_of_block(int R, int T, int& row_tile, int& col_tile) {
    const int L = blockIdx.x;
    if (T % 8 == 0) {
        const int x = L & 7, j = L >> 3;
        row_tile = j % R;
        col_tile = x + 8 * (j / R);
    } else {
        row_tile = L % R;
        col_tile = L / R;
    }
}

// epilogue shared by the tiled GEMM kernels, straight from the accumulators
template <int BM, int BN, int PRO, int EPI>
__device__ __forceinline__ void gemm_epilogue(const LinArgs& a, f4 (&acc)[BM / 32][BN / 32], const float* post, int m0,
                                              int tile0, int wm, int wn, int q, int c) {
    constexpr int WM = BM / 32, WN = BN / 32;
    // ---- epilogue straight from the accumulators.  D layout: column = lane & 15, row = 4 * (lane >> 4) + reg ----
#pragma unroll
    for (int i = 0; i < WM; i++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int mr = (wm * WM + i) * 16 + 4 * q + r;
            const int m = m0 + mr;
            const bool ok = m < a.M;
            const float ps = PRO == PRO_NORM ? post[mr] : 1.0f;
            if (EPI == EPI_SWIGLU) {
#pragma unroll
                for (int j = 0; j < WN; j += 2) {
                    const float g = acc[i][j][r] * ps, u = acc[i][j + 1][r] * ps;
                    const float sg = __fdividef(g, 1.0f + __expf(-g));
                    const int jn = ((tile0 + wn * WN + j) >> 1) * 16 + c;     // column of act[M][N/2]
                    if (ok) a.act[frag_idx(m, jn, a.N / 2)] = sat_half(sg * u);
                }
            } else {
#pragma unroll
                for (int j = 0; j < WN; j++) {
                    const int ng = (tile0 + wn * WN + j) * 16 + c;
                    const float v = acc[i][j][r] * ps;
                    if (EPI == EPI_STORE) {
                        if (ok) a.y[(size_t)m * a.ldy + ng] = v;
                    } else {
                        const size_t hi = frag_idx(m, ng, a.N);
                        const float hn = ok ? a.h_out[hi] + v : 0.f;
                        if (ok) a.h_out[hi] = hn;
                        if (ok && a.xh_out) a.xh_out[hi] = pre_scaled(hn, a.gamma[ng]);
                        const float s2 = group_sum_down<16>(hn * hn);
                        if (ok && c == 0) a.ssq_out[(size_t)m * (a.N / 16) + (ng >> 4)] = s2;
                    }
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------
// gemm_kernel<BM, BN, PRO, EPI> -- the same linear layers for MANY rows (prefill: llama_wrapper.c:125-163 with
// n_tokens = n_text + 9, all utterances of a batch in one ragged pass).  A real tiled GEMM: workgroup = 4 waves
// (2 x 2), tile BM x BN, each wave (BM/2) x (BN/2) as 16x16x32 f16 MFMA fragments; per stage 64 k of the A tile
// (activations, already in fragment order) and of the B tile (weights, fragment order) go global -> registers ->
// LDS, double buffered, one barrier per stage; every fragment is one conflict-free ds_read_b128.  The operands,
// prologue/epilogue semantics and output layouts are exactly linear_kernel's, so the two are interchangeable
// per launch (launch_linear picks by row count).
// ---------------------------------------------------------------------------
template <int BM, int BN, int KS, int PRO, int EPI>
__global__ void __launch_bounds__(256) gemm_kernel(LinArgs a) {
    // KS = k-blocks (32 k each) per stage.  A stage is bounded by the latency of its own global loads (one stage is
    // prefetched while the previous one computes: ~2000 cycles against ~128 * KS cycles of MFMA work), so stages are
    // made as deep as LDS allows: 2 buffers x (BM + BN) / 16 x KS KiB = 128 KiB.
    constexpr int RA = BM / 16, RB = BN / 16;                   // row / column fragments of the tile
    constexpr int NF = (RA + RB) * KS, FPW = NF / 4;            // fragments per stage, per wave to fetch
    constexpr int WM = BM / 32, WN = BN / 32;                   // fragments per wave (rows, columns)
    static_assert(NF % 4 == 0 && WN % 2 == 0, "tile shape");
    Q3_TL(20 + PRO * 4 + EPI);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = w >> 1, wn = w & 1, q = lane >> 4, c = lane & 15;
    int row_tile, col_tile;
    gemm_tile_of_block((a.M - a.m_begin + BM - 1) / BM, a.N / BN, row_tile, col_tile);
    const int m0 = a.m_begin + row_tile * BM;
    const int tile0 = col_tile * RB;
    const int KB = a.K >> 5, NST = KB / KS;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    h8* lds = (h8*)smem;                                        // [2][NF][64] fragments
    __shared__ float post[BM];
    if (PRO == PRO_NORM) {
        for (int r = tid; r < BM; r += 256) {
            const int m = m0 + r;
            float sum = 0.f;
            if (m < a.M) {
                const float4* sp = (const float4*)(a.ssq + (size_t)m * 64);
#pragma unroll
                for (int p = 0; p < 16; p++) {
                    const float4 v = sp[p];
                    sum += (v.x + v.y) + (v.z + v.w);
                }
            }
            post[r] = (1.0f / sqrtf(sum / (float)a.K + a.eps)) * NORM_POST;
        }
    }
    const size_t arow = (size_t)(m0 >> 4) * KB;
    auto frag_ptr = [&](int f, int kb0) -> const h8* {
        if (f < RA * KS) {
            const int rb = f / KS, kk = f % KS;
            return (const h8*)(a.x16 + ((arow + (size_t)rb * KB + kb0 + kk) * 64 + lane) * 8);
        }
        const int g = f - RA * KS, t = g / KS, kk = g % KS;
        return (const h8*)(a.wp + (((size_t)(tile0 + t) * KB + kb0 + kk) * 64 + lane) * 8);
    };
    h8 st[FPW];
#pragma unroll
    for (int i = 0; i < FPW; i++) st[i] = *frag_ptr(w * FPW + i, 0);
#pragma unroll
    for (int i = 0; i < FPW; i++) lds[(w * FPW + i) * 64 + lane] = st[i];
    f4 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; i++)
#pragma unroll
        for (int j = 0; j < WN; j++) acc[i][j] = (f4){0.f, 0.f, 0.f, 0.f};
    __syncthreads();
    for (int ks = 0; ks < NST; ks++) {
        const bool more = ks + 1 < NST;
        if (more) {
#pragma unroll
            for (int i = 0; i < FPW; i++) st[i] = *frag_ptr(w * FPW + i, (ks + 1) * KS);
        }
        const h8* cur = lds + (size_t)(ks & 1) * NF * 64;
#pragma unroll
        for (int kk = 0; kk < KS; kk++) {
            h8 af[WM], bf[WN];
#pragma unroll
            for (int i = 0; i < WM; i++) af[i] = cur[((wm * WM + i) * KS + kk) * 64 + lane];
#pragma unroll
            for (int j = 0; j < WN; j++) bf[j] = cur[(RA * KS + (wn * WN + j) * KS + kk) * 64 + lane];
#pragma unroll
            for (int i = 0; i < WM; i++)
#pragma unroll
                for (int j = 0; j < WN; j++)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        if (more) {
            h8* nxt = lds + (size_t)((ks + 1) & 1) * NF * 64;
#pragma unroll
            for (int i = 0; i < FPW; i++) nxt[(w * FPW + i) * 64 + lane] = st[i];
        }
        __syncthreads();
    }
    gemm_epilogue<BM, BN, PRO, EPI>(a, acc, post, m0, tile0, wm, wn, q, c);
}

// ---------------------------------------------------------------------------
// gemm_glds_kernel<BM, BN, PRO, EPI> -- the same tile GEMM with its operand stream as LDS-DMA
// (global_load_lds_dwordx4: global -> LDS with no VGPR hop) into a ring of NBUF stage buffers, PF stages in flight.
// A stage of gemm_kernel is bounded by the latency of its own loads (~2000 cycles against ~250 cycles of MFMA work
// per 64 k): with M ~ 1000 rows the grid is one workgroup per CU, nothing else hides it.  Here three stages
// (96 KiB per CU for the 128 x 128 tile) are always in flight; a wave waits only for ITS OWN pieces of the stage it
// is about to read (counted s_waitcnt vmcnt), then one raw s_barrier makes the other waves' pieces visible.  The
// fragment order of both operands in global memory is already the lane-linear 1 KiB image LDS-DMA writes.
// ---------------------------------------------------------------------------
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

template <int BM, int BN, int NBUF, int PRO, int EPI, int KS = 2>
__global__ void __launch_bounds__(512) gemm_glds_kernel(LinArgs a) {
    // 8 waves: two groups of 4 (2 x 2 over the tile).  A stage holds KS = 2 k-blocks (64 k); group g multiplies
    // k-block g of every stage, so each SIMD carries two waves whose LDS reads and MFMAs interleave (with one wave
    // per SIMD they alternate: the tile ran at ~2800 cycles per stage against 512 of MFMA work).  The two groups'
    // accumulators meet once, through LDS, in a fixed order (even k-blocks + odd k-blocks).
    constexpr int RA = BM / 16, RB = BN / 16;                   // fragments of the tile; KS k-blocks (32 k) per stage, KS / 2 per group
    static_assert(KS % 2 == 0, "two wave groups share a stage's k-blocks");
    constexpr int NF = (RA + RB) * KS, FPW = NF / 8;            // fragments per stage; per wave to fetch
    constexpr int WM = BM / 32, WN = BN / 32;
    constexpr int PF = NBUF - 1;                                // ring size NBUF; stages in flight
    static_assert(NF % 8 == 0 && WN % 2 == 0, "tile shape");
    static_assert((size_t)NBUF * NF * 1024 >= (size_t)4 * WM * WN * 4 * 64 * 4, "the ring must hold one group's accumulators");
    Q3_TL(24 + PRO * 4 + EPI);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int grp = w >> 2, wq = w & 3;
    const int wm = wq >> 1, wn = wq & 1, q = lane >> 4, c = lane & 15;
    int row_tile, col_tile;
    gemm_tile_of_block((a.M - a.m_begin + BM - 1) / BM, a.N / BN, row_tile, col_tile);
    const int m0 = a.m_begin + row_tile * BM;
    const int tile0 = col_tile * RB;
    const int KB = a.K >> 5, NST = KB / KS;
    extern __shared__ __attribute__((aligned(16))) char smem[];  // ONE LDS object: [NBUF][NF][64] fragments, then post[BM]
    h8* lds = (h8*)smem;
    float* post = (float*)(smem + (size_t)NBUF * NF * 1024);
    const size_t arow = (size_t)(m0 >> 4) * KB;
    auto issue = [&](int st) {       // this wave's FPW pieces of stage st -> ring buffer st % NBUF
        h8* buf = lds + (size_t)(st % NBUF) * NF * 64;
        const int kb0 = st * KS;
#pragma unroll
        for (int i = 0; i < FPW; i++) {
            const int f = w * FPW + i;
            const h8* src;
            if (f < RA * KS) {
                const int rb = f / KS, kk = f % KS;
                src = (const h8*)(a.x16 + ((arow + (size_t)rb * KB + kb0 + kk) * 64 + lane) * 8);
            } else {
                const int g = f - RA * KS, t = g / KS, kk = g % KS;
                src = (const h8*)(a.wp + (((size_t)(tile0 + t) * KB + kb0 + kk) * 64 + lane) * 8);
            }
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(buf + f * 64 + lane), 16, 0, 0);
        }
    };
    // the norm scales first (ordinary loads: the compiler drains them with vmcnt(0) here, before any LDS-DMA exists)
    if (PRO == PRO_NORM) {
        for (int r = tid; r < BM; r += 512) {
            const int m = m0 + r;
            float sum = 0.f;
            if (m < a.M) {
                const float4* sp = (const float4*)(a.ssq + (size_t)m * 64);
#pragma unroll
                for (int p = 0; p < 16; p++) {
                    const float4 v = sp[p];
                    sum += (v.x + v.y) + (v.z + v.w);
                }
            }
            post[r] = (1.0f / sqrtf(sum / (float)a.K + a.eps)) * NORM_POST;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int st = 0; st < PF; st++)
        if (st < NST) issue(st);
    f4 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; i++)
#pragma unroll
        for (int j = 0; j < WN; j++) acc[i][j] = (f4){0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < NST; ks++) {
        // stages issued beyond ks at this point: min(PF - 1, NST - 1 - ks); wait until stage ks (mine) has landed
        const int ahead = NST - 1 - ks;
        if (ahead >= PF - 1) wait_vmcnt<(PF - 1) * FPW>();
        else if (PF > 2 && ahead == 1) wait_vmcnt<FPW>();
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();          // everyone's pieces of stage ks are in LDS; everyone is done with stage ks - 1
        asm volatile("" ::: "memory");
        if (ks + PF < NST) issue(ks + PF);     // into the buffer stage ks - 1 occupied
        const h8* cur = lds + (size_t)(ks % NBUF) * NF * 64;
#pragma unroll
        for (int kk = 0; kk < KS / 2; kk++) {
            const int kb = grp * (KS / 2) + kk;      // this group's k-blocks of the stage
            h8 af[WM], bf[WN];
#pragma unroll
            for (int i = 0; i < WM; i++) af[i] = cur[((wm * WM + i) * KS + kb) * 64 + lane];
#pragma unroll
            for (int j = 0; j < WN; j++) bf[j] = cur[(RA * KS + (wn * WN + j) * KS + kb) * 64 + lane];
#pragma unroll
            for (int i = 0; i < WM; i++)
#pragma unroll
                for (int j = 0; j < WN; j++)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
    }
    // ---- the odd k-blocks' accumulators (group 1) join the even ones (group 0) through the now idle ring ----
    __builtin_amdgcn_s_barrier();              // every wave is done reading the last stage
    asm volatile("" ::: "memory");
    f4* xch = (f4*)smem;                       // [4 waves][WM * WN][64 lanes]
    if (grp == 1) {
#pragma unroll
        for (int i = 0; i < WM; i++)
#pragma unroll
            for (int j = 0; j < WN; j++) xch[((size_t)wq * WM * WN + i * WN + j) * 64 + lane] = acc[i][j];
    }
    __syncthreads();
    if (grp == 1) return;
#pragma unroll
    for (int i = 0; i < WM; i++)
#pragma unroll
        for (int j = 0; j < WN; j++) {
            const f4 o = xch[((size_t)wq * WM * WN + i * WN + j) * 64 + lane];
            acc[i][j] += o;
        }
    gemm_epilogue<BM, BN, PRO, EPI>(a, acc, post, m0, tile0, wm, wn, q, c);
}

// 1 (default): operand stream by LDS-DMA into a 4-stage ring (gemm_glds_kernel); 0: register-staged double buffer
static int g_gemm_glds = env_int("Q3_GEMM_GLDS", 1);
int set_gemm_glds(int on) { g_gemm_glds = on; return 0; }

template <int BM, int BN, int PRO, int EPI>
static int launch_gemm_t(hipStream_t s, const LinArgs& a) {
    LinArgs b = a;
    b.tl_node = tl_next_node();
    dim3 grid(((a.M - a.m_begin + BM - 1) / BM) * (a.N / BN));   // 1-D: the kernels map it to tiles XCD by XCD
    if (g_gemm_glds) {
#ifndef Q3_GEMM_KS_SMALL
#define Q3_GEMM_KS_SMALL 4
#endif
        // (round 3: a 9-deep ring for the 64 x 64 tiles -- 128 KB in flight instead of 48 -- changed nothing, 3.17 vs 3.10 ms
        // per 971-row prefill: those tiles are bound by the per-stage barrier, not by bytes in flight; hence KS below)
        constexpr int NBUF = (BM + BN) > 256 ? 3 : 4;
        constexpr int KS2 = (BM + BN) <= 128 ? Q3_GEMM_KS_SMALL : 2;                        // k-blocks (32 k) per stage
        constexpr size_t lds2 = (size_t)NBUF * ((BM + BN) / 16) * KS2 * 1024 + BM * 4;     // ring + post[BM]
        static bool attr2 = false;
        if (!attr2) {
            Q3_HIP(hipFuncSetAttribute((const void*)gemm_glds_kernel<BM, BN, NBUF, PRO, EPI, KS2>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2), -1);
            attr2 = true;
        }
        if ((a.K >> 5) % KS2) {
            Q3_LOG("launch_gemm: K=%d is no multiple of %d", a.K, 32 * KS2);
            return -1;
        }
        static char name[64];
        if (!name[0])
            snprintf(name, sizeof(name), "gemm_glds<%d,%d,%d,%s,%s,%d>", BM, BN, NBUF, pro_name(PRO), epi_name(EPI), KS2);
        g_last_variant = name;
        hipLaunchKernelGGL((gemm_glds_kernel<BM, BN, NBUF, PRO, EPI, KS2>), grid, dim3(512), lds2, s, b);
    } else if constexpr (BM + BN <= 256) {
        constexpr int KS = 1024 / (BM + BN);    // 128 x 128: 4 k-blocks (128 k) per stage; 64 x 64: 8
        constexpr size_t lds = (size_t)2 * ((BM + BN) / 16) * KS * 1024;
        static bool attr_set = false;
        if (!attr_set) {
            if (lds > 48 * 1024)
                Q3_HIP(hipFuncSetAttribute((const void*)gemm_kernel<BM, BN, KS, PRO, EPI>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), -1);
            attr_set = true;
        }
        static char name[64];
        if (!name[0]) snprintf(name, sizeof(name), "gemm<%d,%d,%d,%s,%s>", BM, BN, KS, pro_name(PRO), epi_name(EPI));
        g_last_variant = name;
        hipLaunchKernelGGL((gemm_kernel<BM, BN, KS, PRO, EPI>), grid, dim3(256), lds, s, b);
    } else {
        // the 128 x 192 tile exists for the LDS-DMA ring only (launch_gemm picks it only with g_gemm_glds): no
        // register-staged instantiation of it is compiled
        Q3_LOG("launch_gemm: no register-staged %d x %d tile", BM, BN);
        return -1;
    }
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

// rows beyond this use the tiled GEMM (buffers are padded to GEMM_ROW_PAD rows)
static int g_gemm_min_rows = 65;
int set_gemm_min_rows(int n) { g_gemm_min_rows = n; return 0; }

static int launch_gemm(hipStream_t s, const LinArgs& a, int pro, int epi) {
    if (a.m_begin % 16 || a.K % 256 || a.N % 128 || (pro == PRO_NORM && a.ssq_parts != 64)) {
        Q3_LOG("launch_gemm: unsupported shape N=%d K=%d m_begin=%d", a.N, a.K, a.m_begin);
        return -1;
    }
    const bool narrow = a.N <= 2048;   // o / down (N = 1024): 64 x 64 tiles, else too few workgroups to fill 256 CUs
    if (pro == PRO_NORM && epi == EPI_STORE) return launch_gemm_t<128, 128, PRO_NORM, EPI_STORE>(s, a);
    if (pro == PRO_NORM && epi == EPI_SWIGLU) {
        // gate/up, N = 6144: 192-column tiles = 32 x 8 = 256 workgroups for ~1000 rows, one per CU, one round
        // (128-column tiles: 384 workgroups, two rounds)
        if (g_gemm_glds && a.N % 192 == 0 && (a.N / 192) % 8 == 0) return launch_gemm_t<128, 192, PRO_NORM, EPI_SWIGLU>(s, a);
        return launch_gemm_t<128, 128, PRO_NORM, EPI_SWIGLU>(s, a);
    }
    if (pro == PRO_F16 && epi == EPI_RESID)
        return narrow ? launch_gemm_t<64, 64, PRO_F16, EPI_RESID>(s, a) : launch_gemm_t<128, 128, PRO_F16, EPI_RESID>(s, a);
    if (pro == PRO_F16 && epi == EPI_STORE)
        return narrow ? launch_gemm_t<64, 64, PRO_F16, EPI_STORE>(s, a) : launch_gemm_t<128, 128, PRO_F16, EPI_STORE>(s, a);
    Q3_LOG("launch_gemm: no instantiation for pro=%d epi=%d", pro, epi);
    return -1;
}

// (round 3 probe: at <= 4 rows -- one utterance -- only the lanes of rows 0-3 fetching activation fragments, compiled in as a
// template variant of linear_kernel and linear_narrow_kernel: 2.145-2.163 against 2.145-2.153 ms per frame, nothing; the
// activation bytes are not what a one-row pass waits for)
template <int NB16, int MT16, int KBW, int NW, int PRO, int EPI>
static int launch_linear_t(hipStream_t s, const LinArgs& a) {
    return a.nt ? launch_linear_nt<NB16, MT16, KBW, NW, PRO, EPI, true>(s, a)
                : launch_linear_nt<NB16, MT16, KBW, NW, PRO, EPI, false>(s, a);
}

// (KBW, NW) per K; overridable for tuning through q3_set_linear_tuning().
static int g_wide_tiles = 0;  // measured no gain on MI355X (4.06 vs 4.12 ms/frame at 32 rows)
int set_linear_wide_tiles(int on) { g_wide_tiles = on; return 0; }
static int g_split_rows_narrow = 1;
int set_linear_split_rows(int on) { g_split_rows_narrow = on; return 0; }
// k-blocks per wave by [K = 1024, 2048, 3072][rows <= 16, <= 32, more]
static const int g_tune_kbw_default[3][3] = {{4, 4, 4}, {16, 8, 8}, {12, 6, 6}};
static int g_tune_kbw[3][3] = {{4, 4, 4}, {16, 8, 8}, {12, 6, 6}};
int set_linear_tuning(int K, int mt16, int kbw) {
    int i = K == 1024 ? 0 : K == 2048 ? 1 : K == 3072 ? 2 : -1;
    int j = mt16 == 1 ? 0 : mt16 == 2 ? 1 : mt16 == 4 ? 2 : -1;
    if (i < 0 || j < 0) return -1;
    g_tune_kbw[i][j] = kbw;
    return 0;
}

// ---------------------------------------------------------------------------
// linear_narrow_kernel<KBW, NW, NT>: the N = 1024 projections (o: K = 2048, down: K = 3072; fp16 input, residual
// epilogue) at <= 64 rows, as their own kernel.  The body of a weight-streaming launch is bound by the bytes each CU
// pulls through its L1 (~77 GB/s per CU), and N = 1024 has only 64 column tiles: with 16-row groups
// a 32-row pass runs 128 workgroups of (16 rows + 16 weight rows) x K x 2 B = 128 / 192 KB each on half the chip.
// Here a workgroup owns 8 rows x 16 columns: 256 workgroups at 32 rows, (8 + 16) x K x 2 B = 96 / 144 KB each, one
// per CU -- and at <= 8 rows (one utterance) the 64 workgroups fetch 8 activation rows instead of 16.  The MFMA is
// still 16 x 16 x 32: lanes of the other 8 rows load nothing (exec-masked, zeros) and their accumulator rows are
// dropped.  Everything else is linear_kernel's EPI_RESID path: every load issued up front, split-K over the NW waves,
// fixed-order LDS reduction, h += acc, 16-column sum-of-squares partials and the consumer's pre-scaled xh.
// Workgroups of one column tile have equal blockIdx.x % 8 (the grid's x extent is 64): one XCD under round-robin
// placement, so the tile's weights come from HBM once and from that L2 for the other row groups.
// ---------------------------------------------------------------------------
template <int KBW, int NW, bool NT>
__global__ void __launch_bounds__(NW * 64)
    linear_narrow_kernel(const half_t* __restrict__ p_wp, const half_t* __restrict__ p_x16, float* __restrict__ p_h,
                         const float* __restrict__ p_gamma, float* __restrict__ p_ssq_out, half_t* __restrict__ p_xh_out,
                         int p_M, int p_m_begin, int tl_node) {
    constexpr int KB = NW * KBW, K = KB * 32, N = 1024, RG = 8;
#ifdef Q3_TIMELINE
    LinArgs a;
    a.tl_node = tl_node;
#endif
    Q3_TL(10 + PRO_F16 * 4 + EPI_RESID);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int q = lane >> 4, c = lane & 15;
    const int tile0 = blockIdx.x;
    const int m0 = p_m_begin + blockIdx.y * RG;          // first row of this group (p_m_begin % 16 == 0)
    const int blk0 = m0 & ~15, half = (m0 >> 3) & 1;     // its 16-row fragment block, and which half of it
    // partial tiles: [wave][4-row group of the 8 rows][column][4 rows] -- a lane's four accumulator registers are
    // four consecutive floats, one ds_write_b128 (as four scalar stores at a row stride of 20 floats the ROCm 7.2
    // compiler merged two of them into a ds_write2_b32 with a wrong first offset -- 5 instead of 20 dwords -- when
    // the accumulators lived in AGPRs: seen in the ISA and in the results of the KBW = 16, NW = 4 instantiation)
    __shared__ __attribute__((aligned(16))) float red[NW * 2 * 16 * 4];
    // ---- every global load of the kernel, up front (epilogue operands first: vmcnt retires in order) ----
    const int mr = tid >> 4, n = tid & 15;               // epilogue mapping: threads 0..127 = 8 rows x 16 columns
    const int m = m0 + mr, ng = tile0 * 16 + n;
    const bool epi_thread = tid < RG * 16, ok = epi_thread && m < p_M;
    float hold = 0.f, gnext = 0.f;
    if (ok) hold = p_h[frag_idx(m, ng, N)];
    if (epi_thread && p_gamma) gnext = p_gamma[ng];
    h8 wf[KBW], af[KBW];
#pragma unroll
    for (int kbi = 0; kbi < KBW; kbi++) {
        const h8* p = (const h8*)(p_wp + (((size_t)tile0 * KB + (size_t)w * KBW + kbi) * 64 + lane) * 8);
        wf[kbi] = NT ? __builtin_nontemporal_load(p) : *p;
    }
    // Lane c holds row blk0 + c of the 16-row block; the lanes of the block's other half fetch nothing.  Their A rows
    // may hold anything (a row of D depends on its own row of A only, and their accumulator rows are dropped), so
    // ONE exec-masked region covers all KBW loads and nothing is merged afterwards.
    const bool live = (c >> 3) == half;
    if (live) {
#pragma unroll
        for (int kbi = 0; kbi < KBW; kbi++)
            af[kbi] = *(const h8*)(p_x16 + frag_idx(blk0 + c, (w * KBW + kbi) * 32 + q * 8, K));
    }
    __builtin_amdgcn_sched_barrier(0);
    Q3_PH(0);  // all loads issued
    f4 acc = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kbi = 0; kbi < KBW; kbi++) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[kbi], wf[kbi], acc, 0, 0, 0);
    Q3_PH(2);  // MFMAs done (weights landed)
    // D layout: col = lane & 15, row = 4 * (lane >> 4) + reg: this group's rows 8 half .. 8 half + 7 sit in q = 2 half, 2 half + 1
    if ((q >> 1) == half) *(f4*)(red + ((w * 2 + (q & 1)) * 16 + c) * 4) = acc;
    __syncthreads();
    Q3_PH(3);
    if (epi_thread) {      // wave-uniform (128 threads = waves 0 and 1)
        float v = 0.f;
#pragma unroll
        for (int ww = 0; ww < NW; ww++) v += red[((ww * 2 + (mr >> 2)) * 16 + n) * 4 + (mr & 3)];
        const float hn = ok ? hold + v : 0.f;
        if (ok) Q3_OUT_STORE(hn, &p_h[frag_idx(m, ng, N)]);
        if (ok && p_xh_out) Q3_OUT_STORE(pre_scaled(hn, gnext), &p_xh_out[frag_idx(m, ng, N)]);
        const float s = group_sum_down<16>(hn * hn);
        if (ok && n == 0) Q3_OUT_STORE(s, &p_ssq_out[(size_t)m * (N / 16) + tile0]);
    }
}

static int g_narrow8 = env_int("Q3_LINEAR_NARROW8", 1);
int set_linear_narrow8(int on) { g_narrow8 = on; return 0; }

template <int KBW, int NW>
static int launch_linear_narrow_t(hipStream_t s, const LinArgs& a) {
    const int groups = (a.M - a.m_begin + 7) / 8;
    const int node = tl_next_node();
    static char name[2][32];
    if (!name[0][0]) {
        snprintf(name[0], sizeof(name[0]), "narrow<%d,%d,t>", KBW, NW);
        snprintf(name[1], sizeof(name[1]), "narrow<%d,%d,nt>", KBW, NW);
    }
    g_last_variant = name[a.nt ? 1 : 0];
    if (a.nt)
        hipLaunchKernelGGL((linear_narrow_kernel<KBW, NW, true>), dim3(64, groups), dim3(NW * 64), 0, s, a.wp, a.x16, a.h_out, a.gamma,
                           a.ssq_out, a.xh_out, a.M, a.m_begin, node);
    else
        hipLaunchKernelGGL((linear_narrow_kernel<KBW, NW, false>), dim3(64, groups), dim3(NW * 64), 0, s, a.wp, a.x16, a.h_out, a.gamma,
                           a.ssq_out, a.xh_out, a.M, a.m_begin, node);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

#define Q3_LIN_CASE(NB16_, MT16_, KBW_, NW_, PRO_, EPI_)                                   \
    if (nb16 == NB16_ && mt16 == MT16_ && kbw == KBW_ && nw == NW_ && pro == PRO_ && epi == EPI_) \
        return launch_linear_t<NB16_, MT16_, KBW_, NW_, PRO_, EPI_>(s, a);

#define Q3_LIN_MT(NB16_, KBW_, NW_, PRO_, EPI_) \
    Q3_LIN_CASE(NB16_, 1, KBW_, NW_, PRO_, EPI_) \
    Q3_LIN_CASE(NB16_, 2, KBW_, NW_, PRO_, EPI_) \
    Q3_LIN_CASE(NB16_, 4, KBW_, NW_, PRO_, EPI_)

// every dispatch knob of launch_linear back to what a fresh process starts with (the two environment defaults re-read)
int reset_linear_knobs() {
    memcpy(g_tune_kbw, g_tune_kbw_default, sizeof(g_tune_kbw));
    g_wide_tiles = 0;
    g_split_rows_narrow = 1;
    g_gemm_min_rows = 65;
    g_narrow8 = env_int("Q3_LINEAR_NARROW8", 1);
    g_gemm_glds = env_int("Q3_GEMM_GLDS", 1);
    return 0;
}

// row tile of linear_kernel (in 16-row blocks) for `rows` rows of an N-column projection
static int decode_mt16(int rows, int N) {
    int mt16 = rows <= 16 ? 1 : rows <= 32 ? 2 : 4;
    // narrow outputs (o/down, N = 1024) have only N/16 = 64 column tiles: split the rows over two
    // workgroups per tile instead (same XCD under round-robin placement, the weights come once from HBM)
    if (rows > 16 && rows <= 32 && ((g_split_rows_narrow == 1 && N <= 1024) || g_split_rows_narrow == 2)) mt16 = 1;
    return mt16;
}

int linear_decode_kbw(int K, int N, int rows) {
    const int ki = K == 1024 ? 0 : K == 2048 ? 1 : K == 3072 ? 2 : -1;
    if (rows <= 0 || rows >= g_gemm_min_rows || ki < 0 || N % 32) return 0;
    const int mt16 = decode_mt16(rows, N);
    return g_tune_kbw[ki][mt16 == 1 ? 0 : mt16 == 2 ? 1 : 2];
}

int launch_linear(hipStream_t s, const LinArgs& a, int pro, int epi) {
    g_last_variant = "";
    const int rows = a.M - a.m_begin;
    if (rows <= 0) return 0;
    if (rows >= g_gemm_min_rows) return launch_gemm(s, a, pro, epi);
    const int K = a.K;
    int ki = K == 1024 ? 0 : K == 2048 ? 1 : K == 3072 ? 2 : -1;
    if (ki < 0 || a.N % 32) {
        Q3_LOG("launch_linear: unsupported shape N=%d K=%d", a.N, K);
        return -1;
    }
    if (g_narrow8 && pro == PRO_F16 && epi == EPI_RESID && a.N == 1024 && a.m_begin % 16 == 0 && a.ssq_out) {
        // o / down: 8-row groups, one workgroup per CU at 32 rows (linear_narrow_kernel)
        // (waves per workgroup probed on MI355X: 4 / 8 / 16 for K = 2048 and 8 / 16 / 4 for K = 3072 all within 0.3 %)
        if (K == 2048) return launch_linear_narrow_t<16, 4>(s, a);
        if (K == 3072) return launch_linear_narrow_t<12, 8>(s, a);
    }
    const int mt16 = decode_mt16(rows, a.N);
    const int kbw = g_tune_kbw[ki][mt16 == 1 ? 0 : mt16 == 2 ? 1 : 2];
    const int nw = K / 32 / kbw;
    // two column tiles per workgroup halve the activation traffic through L2 (it is the larger stream
    // once rows > 16); SwiGLU needs the gate/up pair anyway
    const int nb16 = (epi == EPI_SWIGLU || (g_wide_tiles && rows > 16 && K == 1024 && epi == EPI_STORE)) ? 2 : 1;
    // K = 1024
    Q3_LIN_MT(1, 8, 4, PRO_NORM, EPI_STORE)
    Q3_LIN_MT(1, 4, 8, PRO_NORM, EPI_STORE)
    Q3_LIN_MT(2, 8, 4, PRO_NORM, EPI_SWIGLU)
    Q3_LIN_MT(2, 4, 8, PRO_NORM, EPI_SWIGLU)
    Q3_LIN_MT(1, 8, 4, PRO_F16, EPI_STORE)
    Q3_LIN_MT(2, 4, 8, PRO_NORM, EPI_STORE)
    Q3_LIN_MT(2, 4, 8, PRO_F16, EPI_STORE)
    Q3_LIN_MT(1, 4, 8, PRO_F16, EPI_STORE)
    // K = 2048
    Q3_LIN_MT(1, 8, 8, PRO_F16, EPI_RESID)
    Q3_LIN_MT(1, 4, 16, PRO_F16, EPI_RESID)
    Q3_LIN_MT(1, 16, 4, PRO_F16, EPI_RESID)
    // K = 3072
    Q3_LIN_MT(1, 6, 16, PRO_F16, EPI_RESID)
    Q3_LIN_MT(1, 12, 8, PRO_F16, EPI_RESID)
    Q3_LOG("launch_linear: no instantiation for K=%d kbw=%d nw=%d mt16=%d nb16=%d pro=%d epi=%d", K, kbw, nw,
           mt16, nb16, pro, epi);
    return -1;
}

}  // namespace q3
