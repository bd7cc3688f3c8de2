// q3_test_api.hip -- kernel-level entry points used only by tests/ and bench.py (host arrays in, host arrays
// out).  Built into lib/libqwen3tts_test.so, which links against the product library; NOT part of
// libqwen3tts.so / llama_wrapper.so.
#include "q3_enc.h"
#include "q3_model.h"
#include "q3_spk.h"
#include "q3_voc_ops.h"
#include "q3_xlane.h"
#include <chrono>
#include <cstring>
#include <vector>

using namespace q3;

namespace q3 {
// ---------------------------------------------------------------------------
// test hook of the cross-lane helpers (q3t_xlane_case): one kernel applies a butterfly built on xlane_xor and the same
// butterfly built on __shfl_xor to the same registers.  op 0: sum, 1: max, 2: the (value, index) arg-max exchange of
// block_argmax (index = the element's position in `in`); stages WIDTH/2 .. 1.  n is a multiple of 64 (whole waves, the
// helpers' contract); out_* hold n words, for op 2 another n with the winning indices behind them.
// ---------------------------------------------------------------------------
template <int OP, int WIDTH>
__global__ void __launch_bounds__(256) xlane_case_kernel(const float* __restrict__ in, int n, float* __restrict__ out_new,
                                                         float* __restrict__ out_shfl) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;   // grid * block == n
    const float v = in[i];
    if (OP == 0) {
        out_new[i] = group_sum_down<WIDTH, WIDTH / 2, XlDpp>(v);
        out_shfl[i] = group_sum_down<WIDTH, WIDTH / 2, XlShfl>(v);
    } else if (OP == 1) {
        out_new[i] = group_max_down<WIDTH, WIDTH / 2, XlDpp>(v);
        out_shfl[i] = group_max_down<WIDTH, WIDTH / 2, XlShfl>(v);
    } else {
        float va = v, vb = v;
        int ia = i, ib = i;
        group_argmax_down<WIDTH, WIDTH / 2, XlDpp>(va, ia);
        group_argmax_down<WIDTH, WIDTH / 2, XlShfl>(vb, ib);
        out_new[i] = va;
        out_new[n + i] = __int_as_float(ia);
        out_shfl[i] = vb;
        out_shfl[n + i] = __int_as_float(ib);
    }
}
int launch_xlane_case(hipStream_t s, int op, int width, int n, const float* in, float* out_new, float* out_shfl) {
    if (op < 0 || op > 2 || (width != 4 && width != 16 && width != 64) || n <= 0 || n % 64) return -2;
    const int threads = n % 256 ? 64 : 256;
    const dim3 grid(n / threads), block(threads);
#define Q3_XLANE(OP_, W_)                                                                                   \
    if (op == OP_ && width == W_)                                                                           \
        hipLaunchKernelGGL((xlane_case_kernel<OP_, W_>), grid, block, 0, s, in, n, out_new, out_shfl);
    Q3_XLANE(0, 4) Q3_XLANE(0, 16) Q3_XLANE(0, 64)
    Q3_XLANE(1, 4) Q3_XLANE(1, 16) Q3_XLANE(1, 64)
    Q3_XLANE(2, 4) Q3_XLANE(2, 16) Q3_XLANE(2, 64)
#undef Q3_XLANE
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}
}  // namespace q3

namespace {
struct DBuf {
    void* p = nullptr;
    ~DBuf() {
        if (p) hipFree(p);
    }
    bool alloc(size_t n) { return hipMalloc(&p, n ? n : 16) == hipSuccess; }
    bool up(const void* src, size_t n) { return alloc(n) && (n == 0 || hipMemcpy(p, src, n, hipMemcpyHostToDevice) == hipSuccess); }
};
}  // namespace

extern "C" {

int q3t_set_linear_tuning(int K, int mt16, int kbw) { return set_linear_tuning(K, mt16, kbw); }
int q3t_set_linear_split_rows(int on) { return set_linear_split_rows(on); }
int q3t_set_linear_narrow8(int on) { return set_linear_narrow8(on); }   // 0: o / down through linear_kernel (round 2)
int q3t_set_linear_wide_tiles(int on) { return set_linear_wide_tiles(on); }
int q3t_set_attn_short(int on) { return set_attn_short(on); }
// rows >= n take the tiled GEMM (gemm_kernel) instead of the weight-streaming kernel; default 65
int q3t_set_gemm_min_rows(int n) { return set_gemm_min_rows(n); }
// 1: LDS-DMA ring GEMM (default), 0: the register-staged double-buffer GEMM
int q3t_set_gemm_glds(int on) { return set_gemm_glds(on); }
// every launch_linear dispatch knob back to its start-up value (Q3_LINEAR_NARROW8 / Q3_GEMM_GLDS re-read from the environment)
int q3t_reset_linear_knobs() { return reset_linear_knobs(); }
// the instantiation the last launch_linear call picked, e.g. "linear<1,2,4,8,NORM,STORE,nt>" ("" = it launched nothing)
const char* q3t_last_linear_variant() { return last_linear_variant(); }

// One linear launch.  W is row-major fp16 [N][K]; gateup != 0 means rows [0,N/2) are gate and
// [N/2,N) up (tile-interleaved on the device like the model loader does).
// pro: 0 = x16[M][K] fp16, 1 = RMSNorm(h[M][K], gamma, eps).
// epi: 0 = y[M][N] store, 1 = h_io[M][N] += y with ssq_out[M][N/16], 2 = act_out[M][N/2] fp16.
int q3t_linear(int M, int N, int K, const uint16_t* W, int gateup, int pro, int epi, const uint16_t* x16,
               const float* h, const float* gamma, float eps, float* y_or_h_io, float* ssq_out, uint16_t* act_out,
               int nt) {
    hipStream_t s = nullptr;
    const int Mp = (M + 127) / 128 * 128;  // buffers padded to the largest row tile
    DBuf dW, dWp, dx, dhrows, dh, dssq, dg, dy, dso, dact, dxh;
    if (!dW.up(W, (size_t)N * K * 2) || !dWp.alloc((size_t)N * K * 2)) return -1;
    if (gateup) {
        if (launch_pack_linear(s, (const half_t*)dW.p, N / 2, K, (half_t*)dWp.p, 0, 2)) return -1;
        if (launch_pack_linear(s, (const half_t*)dW.p + (size_t)(N / 2) * K, N / 2, K, (half_t*)dWp.p, 1, 2)) return -1;
    } else {
        if (launch_pack_linear(s, (const half_t*)dW.p, N, K, (half_t*)dWp.p, 0, 1)) return -1;
    }
    LinArgs a;
    a.wp = (const half_t*)dWp.p;
    a.N = N;
    a.K = K;
    a.M = M;
    a.nt = nt;
    if (pro == PRO_F16) {
        std::vector<uint16_t> xp((size_t)Mp * K, 0);   // host rows -> fragment order
        for (int m = 0; m < M; m++)
            for (int k = 0; k < K; k++) xp[frag_idx(m, k, K)] = x16[(size_t)m * K + k];
        if (!dx.up(xp.data(), xp.size() * 2)) return -1;
        a.x16 = (const half_t*)dx.p;
    } else {
        if (!dhrows.up(h, (size_t)M * K * 4) || !dh.alloc((size_t)Mp * K * 4) || !dssq.alloc((size_t)Mp * (K / 16) * 4) ||
            !dg.up(gamma, (size_t)K * 4))
            return -1;
        hipMemset(dh.p, 0, (size_t)Mp * K * 4);
        if (!dxh.alloc((size_t)Mp * K * 2)) return -1;
        hipMemset(dxh.p, 0, (size_t)Mp * K * 2);
        // the producer's side of the folded RMSNorm: h, its sum-of-squares partials and xh = fp16((h*gamma)/16)
        if (launch_ssq_rows(s, (const float*)dhrows.p, (float*)dh.p, (float*)dssq.p, M, K, (half_t*)dxh.p, (const float*)dg.p)) return -1;
        a.x16 = (const half_t*)dxh.p;
        a.ssq = (const float*)dssq.p;
        a.ssq_parts = K / 16;
        a.eps = eps;
    }
    std::vector<float> hp;
    if (epi == EPI_STORE) {
        if (!dy.alloc((size_t)M * N * 4)) return -1;
        a.y = (float*)dy.p;
        a.ldy = N;
    } else if (epi == EPI_RESID) {
        hp.assign((size_t)Mp * N, 0.f);
        for (int m = 0; m < M; m++)
            for (int n = 0; n < N; n++) hp[frag_idx(m, n, N)] = y_or_h_io[(size_t)m * N + n];
        if (!dy.up(hp.data(), hp.size() * 4) || !dso.alloc((size_t)Mp * (N / 16) * 4)) return -1;
        a.h_out = (float*)dy.p;
        a.ssq_out = (float*)dso.p;
    } else {
        if (!dact.alloc((size_t)Mp * (N / 2) * 2)) return -1;
        a.act = (half_t*)dact.p;
    }
    if (launch_linear(s, a, pro, epi)) return -1;
    Q3_HIP(hipDeviceSynchronize(), -1);
    if (epi == EPI_STORE) Q3_HIP(hipMemcpy(y_or_h_io, dy.p, (size_t)M * N * 4, hipMemcpyDeviceToHost), -1);
    if (epi == EPI_RESID) {
        Q3_HIP(hipMemcpy(hp.data(), dy.p, hp.size() * 4, hipMemcpyDeviceToHost), -1);
        for (int m = 0; m < M; m++)
            for (int n = 0; n < N; n++) y_or_h_io[(size_t)m * N + n] = hp[frag_idx(m, n, N)];
        if (ssq_out) Q3_HIP(hipMemcpy(ssq_out, dso.p, (size_t)M * (N / 16) * 4, hipMemcpyDeviceToHost), -1);
    }
    if (epi == EPI_SWIGLU) {
        std::vector<uint16_t> ap((size_t)Mp * (N / 2));
        Q3_HIP(hipMemcpy(ap.data(), dact.p, ap.size() * 2, hipMemcpyDeviceToHost), -1);
        for (int m = 0; m < M; m++)
            for (int j = 0; j < N / 2; j++) act_out[(size_t)m * (N / 2) + j] = ap[frag_idx(m, j, N / 2)];
    }
    return 0;
}

// One linear launch with the whole LinArgs surface, sent through launch_linear the way run_stack sends it: rows
// [m_begin, M) of an M-row buffer are computed.  W is row-major fp16 [N][K] (gateup: rows [0, N/2) gate, [N/2, N) up,
// tile-interleaved on the device like the model loader does).  Host arrays hold rows [0, M), row-major:
//   pro 0 (PRO_F16):  x16[M][K] in.   pro 1 (PRO_NORM): h[M][K], gamma[K] in; launch_ssq_rows produces the GEMM input, and
//                     what it left on the device comes back in pro_h[M][K], pro_ssq[M][K/16], pro_xh[M][K]
//   epi 0: y[M][ldy] out.  epi 1: h_io[M][N] in/out, ssq_out[M][N/16] out, xh_out[M][N] out when gamma_next[N] is given
//   (xh_out without gamma_next, or gamma_next without xh_out: -2).  epi 2: act[M][N/2] out.
// Padding rows of the inputs (>= M) hold finite poison; every output buffer is filled with a NaN sentinel over its
// padded extent first, and -3 is returned when anything outside rows [m_begin, M) x columns [0, N) changed (rows of
// h_io inside keep the caller's values as their start).  Rows [m_begin, M) come back; the others are left as the
// caller passed them.  -2: arguments launch_linear's callers never pass, or no instantiation -- checked before the
// linear launch; -1: a HIP error.
int q3t_linear_case(int M, int m_begin, int N, int K, const uint16_t* W, int gateup, int pro, int epi, int nt, float eps,
                    int ldy, const uint16_t* x16, const float* h, const float* gamma, const float* gamma_next,
                    float* pro_h, float* pro_ssq, uint16_t* pro_xh, float* y, float* h_io, float* ssq_out,
                    uint16_t* xh_out, uint16_t* act) {
    constexpr uint32_t GUARD32 = 0x7fc5a5a5u;   // NaN patterns no kernel produces
    constexpr uint16_t GUARD16 = 0x7d5au;
    constexpr uint16_t POISON16 = 0x7753u;      // fp16 30000: what an unused padding row of an activation may hold
    if (M <= 0 || m_begin < 0 || m_begin >= M || m_begin % 16 || !W) return -2;
    if ((K != 1024 && K != 2048 && K != 3072) || N <= 0 || N % 32) return -2;
    if ((pro != PRO_F16 && pro != PRO_NORM) || (epi != EPI_STORE && epi != EPI_RESID && epi != EPI_SWIGLU)) return -2;
    if (nt != 0 && nt != 1) return -2;
    if (pro == PRO_F16 && !x16) return -2;
    if (pro == PRO_NORM && (!h || !gamma || K != 1024 || !pro_h || !pro_ssq || !pro_xh)) return -2;   // 64 partials per row
    if (epi == EPI_STORE && (!y || ldy < N || gateup)) return -2;
    if (epi == EPI_RESID && (!h_io || !ssq_out || gateup || (xh_out != nullptr) != (gamma_next != nullptr))) return -2;
    if (epi == EPI_SWIGLU && (!act || !gateup || N % 64)) return -2;
    if (epi != EPI_RESID && (xh_out || gamma_next)) return -2;
    hipStream_t s = nullptr;
    const int Mp = m_begin + (M - m_begin + 127) / 128 * 128;   // every row tile of every kernel starts at m_begin
    const int NA = N / 2;
    DBuf dW, dWp, dx, dhrows, dh, dssq, dg, dgn, dy, dho, dso, dxo, dact;
    if (!dW.up(W, (size_t)N * K * 2) || !dWp.alloc((size_t)N * K * 2)) return -1;
    if (gateup) {
        if (launch_pack_linear(s, (const half_t*)dW.p, N / 2, K, (half_t*)dWp.p, 0, 2)) return -1;
        if (launch_pack_linear(s, (const half_t*)dW.p + (size_t)(N / 2) * K, N / 2, K, (half_t*)dWp.p, 1, 2)) return -1;
    } else {
        if (launch_pack_linear(s, (const half_t*)dW.p, N, K, (half_t*)dWp.p, 0, 1)) return -1;
    }
    LinArgs a;
    a.wp = (const half_t*)dWp.p;
    a.N = N;
    a.K = K;
    a.M = M;
    a.m_begin = m_begin;
    a.nt = nt;
    std::vector<uint16_t> xp((size_t)Mp * K, POISON16);
    if (pro == PRO_F16) {
        for (int m = 0; m < M; m++)
            for (int k = 0; k < K; k++) xp[frag_idx(m, k, K)] = x16[(size_t)m * K + k];
        if (!dx.up(xp.data(), xp.size() * 2)) return -1;
        a.x16 = (const half_t*)dx.p;
    } else {
        std::vector<float> hpz((size_t)Mp * K, 3.0e4f), sqz((size_t)Mp * (K / 16), 1.0e9f);
        if (!dhrows.up(h, (size_t)M * K * 4) || !dh.up(hpz.data(), hpz.size() * 4) || !dssq.up(sqz.data(), sqz.size() * 4) ||
            !dx.up(xp.data(), xp.size() * 2) || !dg.up(gamma, (size_t)K * 4))
            return -1;
        // the producer's side of the folded RMSNorm: h, its sum-of-squares partials and xh = fp16((h*gamma)/16)
        if (launch_ssq_rows(s, (const float*)dhrows.p, (float*)dh.p, (float*)dssq.p, M, K, (half_t*)dx.p, (const float*)dg.p)) return -1;
        Q3_HIP(hipDeviceSynchronize(), -1);
        Q3_HIP(hipMemcpy(hpz.data(), dh.p, hpz.size() * 4, hipMemcpyDeviceToHost), -1);
        Q3_HIP(hipMemcpy(xp.data(), dx.p, xp.size() * 2, hipMemcpyDeviceToHost), -1);
        Q3_HIP(hipMemcpy(pro_ssq, dssq.p, (size_t)M * (K / 16) * 4, hipMemcpyDeviceToHost), -1);
        for (int m = 0; m < M; m++)
            for (int k = 0; k < K; k++) {
                pro_h[(size_t)m * K + k] = hpz[frag_idx(m, k, K)];
                pro_xh[(size_t)m * K + k] = xp[frag_idx(m, k, K)];
            }
        a.x16 = (const half_t*)dx.p;
        a.ssq = (const float*)dssq.p;
        a.ssq_parts = K / 16;
        a.eps = eps;
    }
    std::vector<uint32_t> hy, hh, hs;
    std::vector<uint16_t> hx, ha;
    if (epi == EPI_STORE) {
        hy.assign((size_t)Mp * ldy, GUARD32);
        if (!dy.up(hy.data(), hy.size() * 4)) return -1;
        a.y = (float*)dy.p;
        a.ldy = ldy;
    } else if (epi == EPI_RESID) {
        hh.assign((size_t)Mp * N, GUARD32);
        hs.assign((size_t)Mp * (N / 16), GUARD32);
        for (int m = m_begin; m < M; m++)
            for (int n = 0; n < N; n++) memcpy(&hh[frag_idx(m, n, N)], &h_io[(size_t)m * N + n], 4);
        if (!dho.up(hh.data(), hh.size() * 4) || !dso.up(hs.data(), hs.size() * 4)) return -1;
        a.h_out = (float*)dho.p;
        a.ssq_out = (float*)dso.p;
        if (xh_out) {
            hx.assign((size_t)Mp * N, GUARD16);
            if (!dxo.up(hx.data(), hx.size() * 2) || !dgn.up(gamma_next, (size_t)N * 4)) return -1;
            a.xh_out = (half_t*)dxo.p;
            a.gamma = (const float*)dgn.p;
        }
    } else {
        ha.assign((size_t)Mp * NA, GUARD16);
        if (!dact.up(ha.data(), ha.size() * 2)) return -1;
        a.act = (half_t*)dact.p;
    }
    Q3_HIP(hipDeviceSynchronize(), -1);
    if (launch_linear(s, a, pro, epi)) {
        // refused before its launch (no instantiation for this shape under the current knobs): nothing ran
        if (!last_linear_variant()[0] && hipGetLastError() == hipSuccess) return -2;
        return -1;
    }
    Q3_HIP(hipDeviceSynchronize(), -1);
    auto inside = [&](int m) { return m >= m_begin && m < M; };
    int outside = 0;
    if (epi == EPI_STORE) {
        Q3_HIP(hipMemcpy(hy.data(), dy.p, hy.size() * 4, hipMemcpyDeviceToHost), -1);
        for (int m = 0; m < Mp; m++)
            for (int n = 0; n < ldy; n++) {
                const uint32_t v = hy[(size_t)m * ldy + n];
                if (inside(m) && n < N) memcpy(&y[(size_t)m * ldy + n], &v, 4);
                else if (v != GUARD32) outside++;
            }
    } else if (epi == EPI_RESID) {
        Q3_HIP(hipMemcpy(hh.data(), dho.p, hh.size() * 4, hipMemcpyDeviceToHost), -1);
        Q3_HIP(hipMemcpy(hs.data(), dso.p, hs.size() * 4, hipMemcpyDeviceToHost), -1);
        if (xh_out) Q3_HIP(hipMemcpy(hx.data(), dxo.p, hx.size() * 2, hipMemcpyDeviceToHost), -1);
        for (int m = 0; m < Mp; m++) {
            for (int n = 0; n < N; n++) {
                const size_t fi = frag_idx(m, n, N);
                if (inside(m)) {
                    memcpy(&h_io[(size_t)m * N + n], &hh[fi], 4);
                    if (xh_out) xh_out[(size_t)m * N + n] = hx[fi];
                } else if (hh[fi] != GUARD32 || (xh_out && hx[fi] != GUARD16)) {
                    outside++;
                }
            }
            for (int p = 0; p < N / 16; p++) {
                const uint32_t v = hs[(size_t)m * (N / 16) + p];
                if (inside(m)) memcpy(&ssq_out[(size_t)m * (N / 16) + p], &v, 4);
                else if (v != GUARD32) outside++;
            }
        }
    } else {
        Q3_HIP(hipMemcpy(ha.data(), dact.p, ha.size() * 2, hipMemcpyDeviceToHost), -1);
        for (int m = 0; m < Mp; m++)
            for (int j = 0; j < NA; j++) {
                const uint16_t v = ha[frag_idx(m, j, NA)];
                if (inside(m)) act[(size_t)m * NA + j] = v;
                else if (v != GUARD16) outside++;
            }
    }
    return outside ? -3 : 0;
}

// One attention call of the talker / code-predictor shape (16 q heads, 8 kv heads, head_dim 128) on host arrays, sent
// through launch_attn the way run_stack sends it.  mode 0: ATTN_FUSED; mode 1: ATTN_PREP then ATTN_ATTEND (tiles /
// n_tiles as run_stack passes them: explicit tiles {first row, rows, slot, first position}, or tiles == null with
// n_tiles = (R + 15) / 16 for one implicit run).  Rows row0 .. row0+R-1 are computed: qkv[R][4096] (f32), slot / pos
// [R] (or null: *_base + r * *_stride, r counted from row 0) and out[R][2048] (fp16, row-major, in/out: rows the call
// skips keep what was uploaded) hold those rows; tile rows are absolute (row0 .. row0+R-1).  Caches kc / vc
// [n_slots][8][n_ctx][128] fp16 are uploaded and returned; rope tables are [max_pos][64].  Every row and tile is
// checked against the buffers before anything launches (-2); -3: the launch wrote outside rows row0 .. row0+R-1.
int q3t_attn(int mode, int R, int row0, const float* qkv, const float* q_norm, const float* k_norm, float eps,
             const float* rope_cos, const float* rope_sin, int max_pos, const int* slot, const int* pos, int slot_base,
             int slot_stride, int pos_base, int pos_stride, uint16_t* kc, uint16_t* vc, int n_slots, int n_ctx,
             const int* tiles, int n_tiles, int valid_mod, int valid_n, int threads, uint16_t* out) {
    constexpr int NH = 16, NKV = 8, D = 128, LD = (NH + 2 * NKV) * D, OW = NH * D;
    constexpr uint16_t GUARD = 0x7d5au;   // a NaN pattern in the rows outside the call (the kernels never produce it)
    if (mode != 0 && mode != 1) return -2;
    if (R <= 0 || row0 < 0 || !qkv || !q_norm || !k_norm || !rope_cos || !rope_sin || !kc || !vc || !out) return -2;
    if (max_pos <= 0 || n_slots <= 0 || n_ctx <= 0 || threads < 64 || threads > 1024 || threads % 64) return -2;
    if (valid_mod < 0 || (valid_mod > 0 && (valid_n < 0 || valid_n > valid_mod))) return -2;
    const int rows = row0 + R;
    auto skipped = [&](int r) { return valid_mod > 0 && (r % valid_mod) >= valid_n; };
    auto row_slot = [&](int r) { return slot ? slot[r - row0] : slot_base + r * slot_stride; };
    auto row_pos = [&](int r) { return pos ? pos[r - row0] : pos_base + r * pos_stride; };
    // every row the kernels touch: its cache row (written) and its rope row (read)
    for (int r = row0; r < rows; r++) {
        if (skipped(r)) continue;
        const int sl = row_slot(r), p = row_pos(r);
        if (sl < 0 || sl >= n_slots || p < 0 || p >= n_ctx || p >= max_pos) return -2;
    }
    if (mode == 0) {
        if (n_tiles != 0 || tiles) return -2;
        // two rows appending to one slot in one FUSED call race (run_stack sends those through PREP + ATTEND)
        std::vector<char> seen((size_t)n_slots, 0);
        for (int r = row0; r < rows; r++) {
            if (skipped(r)) continue;
            if (seen[(size_t)row_slot(r)]++) return -2;
        }
    } else if (n_tiles > 0 && !tiles) {
        // one implicit run: the form run_stack tiles implicitly, nothing else
        if (slot || pos || slot_stride != 0 || pos_stride != 1 || valid_mod != 0 || n_tiles != (R + 15) / 16) return -2;
    } else if (n_tiles > 0) {
        for (int i = 0; i < n_tiles; i++) {
            const int* t = tiles + 4 * i;
            if (t[0] < row0 || t[1] < 1 || t[1] > 16 || t[0] + t[1] > rows) return -2;
            if (t[2] < 0 || t[2] >= n_slots || t[3] < 0 || t[3] + t[1] > n_ctx) return -2;
        }
    } else if (n_tiles < 0 || tiles) {
        return -2;
    }
    hipStream_t s = nullptr;
    const int Rp = (rows + 15) / 16 * 16;   // the output's fragment order is padded to 16 rows
    const size_t cache = (size_t)n_slots * NKV * n_ctx * D;
    std::vector<float> hq((size_t)Rp * LD, 0.f);
    memcpy(hq.data() + (size_t)row0 * LD, qkv, (size_t)R * LD * 4);
    std::vector<uint16_t> ho((size_t)Rp * OW, GUARD);
    for (int r = row0; r < rows; r++)
        for (int k = 0; k < OW; k++) ho[frag_idx(r, k, OW)] = out[(size_t)(r - row0) * OW + k];
    std::vector<int> hs((size_t)Rp, 0), hp((size_t)Rp, 0);
    for (int r = row0; r < rows; r++) {
        if (slot) hs[r] = slot[r - row0];
        if (pos) hp[r] = pos[r - row0];
    }
    DBuf dq, dqn, dkn, dcs, dsn, dkc, dvc, dout, dslot, dpos, dtiles;
    if (!dq.up(hq.data(), hq.size() * 4) || !dqn.up(q_norm, D * 4) || !dkn.up(k_norm, D * 4) ||
        !dcs.up(rope_cos, (size_t)max_pos * 64 * 4) || !dsn.up(rope_sin, (size_t)max_pos * 64 * 4) ||
        !dkc.up(kc, cache * 2) || !dvc.up(vc, cache * 2) || !dout.up(ho.data(), ho.size() * 2) ||
        !dslot.up(hs.data(), hs.size() * 4) || !dpos.up(hp.data(), hp.size() * 4))
        return -1;
    if (tiles && !dtiles.up(tiles, (size_t)n_tiles * 16)) return -1;
    AttnArgs t;
    t.qkv = (float*)dq.p;
    t.ld = LD;
    t.R = R;
    t.row0 = row0;
    t.q_norm = (const float*)dqn.p;
    t.k_norm = (const float*)dkn.p;
    t.eps = eps;
    t.rope_cos = (const float*)dcs.p;
    t.rope_sin = (const float*)dsn.p;
    t.slot = slot ? (const int*)dslot.p : nullptr;
    t.pos = pos ? (const int*)dpos.p : nullptr;
    t.slot_base = slot_base;
    t.slot_stride = slot_stride;
    t.pos_base = pos_base;
    t.pos_stride = pos_stride;
    t.kc = (half_t*)dkc.p;
    t.vc = (half_t*)dvc.p;
    t.n_ctx = n_ctx;
    t.n_kv = NKV;
    t.n_heads = NH;
    t.out = (half_t*)dout.p;
    t.scale = 1.0f / sqrtf((float)D);
    t.threads = threads;
    t.valid_mod = valid_mod;
    t.valid_n = valid_n;
    if (mode == 0) {
        if (launch_attn(s, t, ATTN_FUSED)) return -1;
    } else {
        if (launch_attn(s, t, ATTN_PREP)) return -1;
        t.tiles = tiles ? (const int*)dtiles.p : nullptr;
        t.n_tiles = n_tiles;
        if (launch_attn(s, t, ATTN_ATTEND)) return -1;
    }
    Q3_HIP(hipDeviceSynchronize(), -1);
    Q3_HIP(hipMemcpy(kc, dkc.p, cache * 2, hipMemcpyDeviceToHost), -1);
    Q3_HIP(hipMemcpy(vc, dvc.p, cache * 2, hipMemcpyDeviceToHost), -1);
    Q3_HIP(hipMemcpy(ho.data(), dout.p, ho.size() * 2, hipMemcpyDeviceToHost), -1);
    for (int r = row0; r < rows; r++)
        for (int k = 0; k < OW; k++) out[(size_t)(r - row0) * OW + k] = ho[frag_idx(r, k, OW)];
    for (int r = 0; r < Rp; r++) {
        if (r >= row0 && r < rows) continue;
        for (int k = 0; k < OW; k++)
            if (ho[frag_idx(r, k, OW)] != GUARD) return -3;
    }
    return 0;
}

// The vocoder's sliding-window RoPE attention on host arrays: x[B][3*H*D][L] (q | k | v, head-major rows of L columns)
// -> y[B][H*D][L].  kernel 0: voc_attn_kernel (any even D <= 128), 1: voc_attn_tile_kernel (the launcher refuses shapes it
// does not hold).  The device rows have the vocoder's pitch (L rounded up to 32 floats); -3: a pad column was written.
int q3t_voc_attn(int kernel, const float* x, float* y, int B, int H, int D, int L, int window, float theta) {
    constexpr float GUARD = 1234.5f;
    if ((kernel != 0 && kernel != 1) || !x || !y || B <= 0 || H <= 0 || D <= 0 || D > 128 || (D & 1) || L <= 0 || window <= 0)
        return -2;
    const int ld = (L + 31) / 32 * 32;
    const size_t nx = (size_t)B * 3 * H * D, ny = (size_t)B * H * D;
    std::vector<float> hx(nx * ld, 0.f), hy(ny * ld, GUARD);
    for (size_t r = 0; r < nx; r++) memcpy(hx.data() + r * ld, x + r * L, (size_t)L * 4);
    DBuf dx, dy;
    if (!dx.up(hx.data(), hx.size() * 4) || !dy.up(hy.data(), hy.size() * 4)) return -1;
    const int rc = kernel == 0 ? voc_launch_attn(nullptr, (const float*)dx.p, (float*)dy.p, H, D, L, ld, window, theta, B)
                               : voc_launch_attn_tile(nullptr, (const float*)dx.p, (float*)dy.p, H, D, L, ld, window, theta, B);
    if (rc) return -2;
    Q3_HIP(hipDeviceSynchronize(), -1);
    Q3_HIP(hipMemcpy(hy.data(), dy.p, hy.size() * 4, hipMemcpyDeviceToHost), -1);
    for (size_t r = 0; r < ny; r++) {
        memcpy(y + r * L, hy.data() + r * ld, (size_t)L * 4);
        for (int l = L; l < ld; l++)
            if (hy[r * ld + l] != GUARD) return -3;
    }
    return 0;
}

// The cross-lane helpers of q3_xlane.h (xlane_xor) against __shfl_xor, both applied to the same registers by one
// kernel.  op 0: sum, 1: max, 2: the (value, index) arg-max exchange of block_argmax; width 4, 16 or 64 lanes; n values
// (a multiple of 64).  out_new / out_shfl: n words each, for op 2 another n int32 words (the winning indices) behind them.
int q3t_xlane_case(int op, int width, int n, const float* in, float* out_new, float* out_shfl) {
    if (!in || !out_new || !out_shfl || n <= 0 || n % 64) return -2;
    const size_t words = (size_t)n * (op == 2 ? 2 : 1);
    DBuf din, da, db;
    if (!din.up(in, (size_t)n * 4) || !da.alloc(words * 4) || !db.alloc(words * 4)) return -1;
    const int rc = launch_xlane_case(nullptr, op, width, n, (const float*)din.p, (float*)da.p, (float*)db.p);
    if (rc) return rc;
    Q3_HIP(hipDeviceSynchronize(), -1);
    Q3_HIP(hipMemcpy(out_new, da.p, words * 4, hipMemcpyDeviceToHost), -1);
    Q3_HIP(hipMemcpy(out_shfl, db.p, words * 4, hipMemcpyDeviceToHost), -1);
    return 0;
}

// Time `iters` back-to-back launches of one linear shape over `n_copies` distinct weight copies
// (cold weights like the real layer walk).  Returns average microseconds per launch, <0 on error.
float q3t_bench_linear(int M, int N, int K, int pro, int epi, int nt, int n_copies, int iters) {
    hipStream_t s = nullptr;
    if (hipStreamCreate(&s) != hipSuccess) return -1.f;
    const size_t wbytes = (size_t)N * K * 2;
    const int Mreal = M;
    M = (M + 127) / 128 * 128;  // allocation padding; the launch uses Mreal rows
    DBuf dW, dx, dh, dssq, dg, dy, dso, dact;
    if (!dW.alloc(wbytes * n_copies)) return -1.f;
    hipMemset(dW.p, 0x11, wbytes * n_copies);
    dx.alloc((size_t)M * K * 2);
    hipMemset(dx.p, 0, (size_t)M * K * 2);
    dh.alloc((size_t)M * K * 4);
    hipMemset(dh.p, 0, (size_t)M * K * 4);
    dssq.alloc((size_t)M * (K / 16) * 4);
    hipMemset(dssq.p, 0, (size_t)M * (K / 16) * 4);
    dg.alloc((size_t)K * 4);
    hipMemset(dg.p, 0, (size_t)K * 4);
    dy.alloc((size_t)M * N * 4);
    dso.alloc((size_t)M * (N / 16) * 4);
    dact.alloc((size_t)M * (N / 2) * 2);
    LinArgs a;
    a.N = N;
    a.K = K;
    a.M = Mreal;
    a.nt = nt;
    a.x16 = (const half_t*)dx.p;
    a.ssq = (const float*)dssq.p;
    a.ssq_parts = K / 16;
    a.y = (float*)dy.p;
    a.ldy = N;
    a.h_out = (float*)dy.p;
    a.ssq_out = (float*)dso.p;
    a.act = (half_t*)dact.p;
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    for (int it = -n_copies; it < iters; it++) {
        if (it == 0) hipEventRecord(e0, s);
        a.wp = (const half_t*)((char*)dW.p + wbytes * (size_t)((it + n_copies) % n_copies));
        if (launch_linear(s, a, pro, epi)) return -1.f;
    }
    hipEventRecord(e1, s);
    if (hipStreamSynchronize(s) != hipSuccess) return -1.f;
    float ms = 0.f;
    hipEventElapsedTime(&ms, e0, e1);
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    hipStreamDestroy(s);
    return ms * 1000.f / iters;
}

}  // extern "C"

// Talker sampling kernel on host arrays: logits[V], the chronological list of already emitted
// code_0 (n_past entries), n_text.  Returns the emitted code, or -1 when the utterance ends
// (EOS / non-audio id / forced EOS); -1000 on error.
extern "C" int q3t_talker_sample(const float* logits, int V, const int* past, int n_past, int n_text, int ignore_eos) {
    DBuf dl, dpast, dn, dnt, ddone, dcodes, dnf, dpos0, dpos;
    int ring[32] = {0};
    for (int i = n_past > 32 ? n_past - 32 : 0; i < n_past; i++) ring[i & 31] = past[i];
    int zero = 0, pos0 = 7;
    if (!dl.up(logits, (size_t)V * 4) || !dpast.up(ring, sizeof(ring)) || !dn.up(&n_past, 4) || !dnt.up(&n_text, 4) ||
        !ddone.up(&zero, 4) || !dcodes.alloc(16 * 4) || !dnf.up(&zero, 4) || !dpos0.up(&pos0, 4) || !dpos.up(&zero, 4))
        return -1000;
    TalkerSampleArgs a;
    a.logits = (const float*)dl.p;
    a.V = V;
    a.R = 1;
    a.past = (int*)dpast.p;
    a.n_past = (int*)dn.p;
    a.n_text = (const int*)dnt.p;
    a.done = (int*)ddone.p;
    a.codes = (int*)dcodes.p;
    a.n_frames = (int*)dnf.p;
    a.frame_cap = 1;
    a.pos0 = (const int*)dpos0.p;
    a.pos = (int*)dpos.p;
    a.ignore_eos = ignore_eos;
    if (launch_talker_sample(nullptr, a)) return -1000;
    int code = -1000;
    if (hipDeviceSynchronize() != hipSuccess) return -1000;
    if (hipMemcpy(&code, dcodes.p, 4, hipMemcpyDeviceToHost) != hipSuccess) return -1000;
    return code;
}

// One launch_talker_sample over rows row0 .. row0+R-1 of a batch of R_total, every piece of state in and out on host
// arrays: logits[R_total][V], past[R_total][32], n_past / n_text / done / n_frames / pos0 / pos [R_total],
// codes[frame_cap][R_total][16], forced (same layout, or null), seed_ptr[R_total] (or null), slots = SlotParams[R_total]
// (or null; non-null selects the per-slot kernel).  Returns the launcher's own refusal (-1), -2 for arguments this hook
// cannot lay out, -1000 on a HIP error.
static int talker_sample_case(const float* logits, int V, int R_total, int row0, int R, int* past, int* n_past,
                              const int* n_text, int* done, int* n_frames, const int* pos0, int* pos, int* codes,
                              int frame_cap, const int* forced, int audio_vocab, int eos, int ignore_eos, int max_frames,
                              float rep_penalty, float temperature, int top_k, float top_p, unsigned long long seed,
                              const unsigned long long* seed_ptr, const void* slots, const int* text_avail, int* held,
                              const void* rules = nullptr, unsigned* seen = nullptr, float* scores = nullptr) {
    if (!logits || V <= 0 || R < 0 || row0 < 0 || row0 + R > R_total || frame_cap < 0 || eos < 0 || eos >= V) return -2;
    if (seen && audio_vocab <= 0) return -2;
    const size_t seen_words = seen ? (size_t)R_total * ((audio_vocab + 31) / 32) : 0;
    for (int r = row0; r < row0 + R; r++)
        if (n_frames[r] < 0 || n_past[r] < 0) return -2;
    const size_t rt = (size_t)R_total, nc = (size_t)frame_cap * rt * 16;
    DBuf dl, dpast, dn, dnt, ddone, dcodes, dnf, dpos0, dpos, dforced, dseed, dslots, dtav, dheld, drules, dseen, dscores;
    if (scores && !dscores.up(scores, nc * 4)) return -1000;
    if (rules && !drules.up(rules, rt * sizeof(SlotRules))) return -1000;
    if (seen && !dseen.up(seen, seen_words * 4)) return -1000;
    if (text_avail && !dtav.up(text_avail, rt * 4)) return -1000;
    if (held && !dheld.up(held, rt * 4)) return -1000;
    if (!dl.up(logits, rt * V * 4) || !dpast.up(past, rt * 32 * 4) || !dn.up(n_past, rt * 4) || !dnt.up(n_text, rt * 4) ||
        !ddone.up(done, rt * 4) || !dcodes.up(codes, nc * 4) || !dnf.up(n_frames, rt * 4) || !dpos0.up(pos0, rt * 4) ||
        !dpos.up(pos, rt * 4))
        return -1000;
    if (forced && !dforced.up(forced, nc * 4)) return -1000;
    if (seed_ptr && !dseed.up(seed_ptr, rt * 8)) return -1000;
    if (slots && !dslots.up(slots, rt * sizeof(SlotParams))) return -1000;
    TalkerSampleArgs a;
    a.logits = (const float*)dl.p;
    a.V = V;
    a.R = R;
    a.row0 = row0;
    a.R_total = R_total;
    a.audio_vocab = audio_vocab;
    a.eos = eos;
    a.past = (int*)dpast.p;
    a.n_past = (int*)dn.p;
    a.n_text = (const int*)dnt.p;
    a.done = (int*)ddone.p;
    a.codes = (int*)dcodes.p;
    a.n_frames = (int*)dnf.p;
    a.frame_cap = frame_cap;
    a.pos0 = (const int*)dpos0.p;
    a.pos = (int*)dpos.p;
    a.ignore_eos = ignore_eos;
    a.max_frames = max_frames;
    a.rep_penalty = rep_penalty;
    a.temperature = temperature;
    a.top_p = top_p;
    a.top_k = top_k;
    a.seed = seed;
    a.seed_ptr = seed_ptr ? (const unsigned long long*)dseed.p : nullptr;
    a.forced = forced ? (const int*)dforced.p : nullptr;
    a.slots = slots ? (const SlotParams*)dslots.p : nullptr;
    a.text_avail = text_avail ? (const int*)dtav.p : nullptr;
    a.held = held ? (int*)dheld.p : nullptr;
    a.rules = rules ? (const SlotRules*)drules.p : nullptr;
    a.seen = seen ? (unsigned*)dseen.p : nullptr;
    a.scores = scores ? (float*)dscores.p : nullptr;
    if (const int rc = launch_talker_sample(nullptr, a)) return rc;
    Q3_HIP(hipDeviceSynchronize(), -1000);
    Q3_HIP(hipMemcpy(past, dpast.p, rt * 32 * 4, hipMemcpyDeviceToHost), -1000);
    Q3_HIP(hipMemcpy(n_past, dn.p, rt * 4, hipMemcpyDeviceToHost), -1000);
    Q3_HIP(hipMemcpy(done, ddone.p, rt * 4, hipMemcpyDeviceToHost), -1000);
    Q3_HIP(hipMemcpy(n_frames, dnf.p, rt * 4, hipMemcpyDeviceToHost), -1000);
    Q3_HIP(hipMemcpy(pos, dpos.p, rt * 4, hipMemcpyDeviceToHost), -1000);
    Q3_HIP(hipMemcpy(codes, dcodes.p, nc * 4, hipMemcpyDeviceToHost), -1000);
    if (held) Q3_HIP(hipMemcpy(held, dheld.p, rt * 4, hipMemcpyDeviceToHost), -1000);
    if (seen) Q3_HIP(hipMemcpy(seen, dseen.p, seen_words * 4, hipMemcpyDeviceToHost), -1000);
    if (scores) Q3_HIP(hipMemcpy(scores, dscores.p, nc * 4, hipMemcpyDeviceToHost), -1000);
    return 0;
}
extern "C" int q3t_talker_sample_case(const float* logits, int V, int R_total, int row0, int R, int* past, int* n_past,
                                      const int* n_text, int* done, int* n_frames, const int* pos0, int* pos, int* codes,
                                      int frame_cap, const int* forced, int audio_vocab, int eos, int ignore_eos,
                                      int max_frames, float rep_penalty, float temperature, int top_k, float top_p,
                                      unsigned long long seed, const unsigned long long* seed_ptr, const void* slots) {
    return talker_sample_case(logits, V, R_total, row0, R, past, n_past, n_text, done, n_frames, pos0, pos, codes, frame_cap,
                              forced, audio_vocab, eos, ignore_eos, max_frames, rep_penalty, temperature, top_k, top_p, seed,
                              seed_ptr, slots, nullptr, nullptr);
}
// q3t_talker_sample_case with held text slots (TalkerSampleArgs::text_avail / held): text_avail[R_total] in, held[R_total]
// in and out, whole -- rows outside the launch come back as they went in.  Either may be null (the launcher's refusals).
extern "C" int q3t_talker_sample_text_case(const float* logits, int V, int R_total, int row0, int R, int* past, int* n_past,
                                           const int* n_text, int* done, int* n_frames, const int* pos0, int* pos, int* codes,
                                           int frame_cap, const int* forced, int audio_vocab, int eos, int ignore_eos,
                                           int max_frames, float rep_penalty, float temperature, int top_k, float top_p,
                                           unsigned long long seed, const unsigned long long* seed_ptr, const void* slots,
                                           const int* text_avail, int* held) {
    return talker_sample_case(logits, V, R_total, row0, R, past, n_past, n_text, done, n_frames, pos0, pos, codes, frame_cap,
                              forced, audio_vocab, eos, ignore_eos, max_frames, rep_penalty, temperature, top_k, top_p, seed,
                              seed_ptr, slots, text_avail, held);
}
// q3t_talker_sample_text_case with sampler rules (TalkerSampleArgs::rules / seen): rules = SlotRules[R_total] in,
// seen[R_total][(audio_vocab + 31) / 32] in and out, whole.  Either may be null (the launcher's refusals).
extern "C" int q3t_talker_sample_rules_case(const float* logits, int V, int R_total, int row0, int R, int* past, int* n_past,
                                            const int* n_text, int* done, int* n_frames, const int* pos0, int* pos, int* codes,
                                            int frame_cap, const int* forced, int audio_vocab, int eos, int ignore_eos,
                                            int max_frames, float rep_penalty, float temperature, int top_k, float top_p,
                                            unsigned long long seed, const unsigned long long* seed_ptr, const void* slots,
                                            const int* text_avail, int* held, const void* rules, unsigned* seen) {
    return talker_sample_case(logits, V, R_total, row0, R, past, n_past, n_text, done, n_frames, pos0, pos, codes, frame_cap,
                              forced, audio_vocab, eos, ignore_eos, max_frames, rep_penalty, temperature, top_k, top_p, seed,
                              seed_ptr, slots, text_avail, held, rules, seen);
}

// q3t_talker_sample_rules_case with the log-probability of the id the stream continues with (TalkerSampleArgs::scores):
// scores[frame_cap][R_total][16] in and out, whole -- entries the launch leaves alone come back as they went in.  Null:
// q3t_talker_sample_rules_case itself.
extern "C" int q3t_talker_score_case(const float* logits, int V, int R_total, int row0, int R, int* past, int* n_past,
                                     const int* n_text, int* done, int* n_frames, const int* pos0, int* pos, int* codes,
                                     int frame_cap, const int* forced, int audio_vocab, int eos, int ignore_eos,
                                     int max_frames, float rep_penalty, float temperature, int top_k, float top_p,
                                     unsigned long long seed, const unsigned long long* seed_ptr, const void* slots,
                                     const int* text_avail, int* held, const void* rules, unsigned* seen, float* scores) {
    return talker_sample_case(logits, V, R_total, row0, R, past, n_past, n_text, done, n_frames, pos0, pos, codes, frame_cap,
                              forced, audio_vocab, eos, ignore_eos, max_frames, rep_penalty, temperature, top_k, top_p, seed,
                              seed_ptr, slots, text_avail, held, rules, seen, scores);
}

// One launch_cp_argmax, state in and out on host arrays (layouts as in q3t_talker_sample_case).  epilogue 0: none;
// 1: gather of next_table[V][H] (+ next_qkv[V][qkv_ld] -> qkv_out[R_total][qkv_ld] when non-null); 2: the feedback sum
// over talker_emb[talker_vocab][H], cp_tables[n_groups][V][H] (one contiguous array) and pad[H] (or null).
// h_out[R_total][H], ssq_out[R_total][H/16] and xh_out[R_total][H] (fp16 bits; with gamma[H], or both null) are row-major
// in and out: the hook lays them out in fragment order on the device, so rows the launch leaves alone keep what the
// caller put there.  Returns as q3t_talker_sample_case.
static int cp_sample_case(const float* logits, int V, int R_total, int row0, int R, int group, int* codes,
                          const int* n_frames, int frame_cap, const int* forced, float temperature, int top_k,
                          unsigned long long seed, const unsigned long long* seed_ptr, const void* slots, int epilogue, int H,
                          const float* next_table, const float* next_qkv, int qkv_ld, const float* gamma,
                          const float* talker_emb, int talker_vocab, const float* cp_tables, int n_groups, const float* pad,
                          float* h_out, float* ssq_out, uint16_t* xh_out, float* qkv_out, const float* text_rows,
                          const int* text_avail, int text_cap, const int* held, const void* rules = nullptr,
                          float* scores = nullptr) {
    if (!logits || V <= 0 || R < 0 || row0 < 0 || row0 + R > R_total || frame_cap < 1 || group < 0 || group > 14 ||
        epilogue < 0 || epilogue > 2)
        return -2;
    for (int r = row0; r < row0 + R; r++)
        if (n_frames[r] < 0) return -2;
    if (epilogue) {
        if (H <= 0 || H % 32 || !h_out || !ssq_out || (xh_out != nullptr) != (gamma != nullptr)) return -2;
        if (epilogue == 1 && (!next_table || (next_qkv && (!qkv_out || qkv_ld <= 0 || qkv_ld % 4)))) return -2;
        if (epilogue == 2 && (!talker_emb || talker_vocab <= 0 || !cp_tables || n_groups <= group || n_groups > 15)) return -2;
    }
    // a text row is read at [r][n_frames - 1] while n_frames - 1 < text_avail[r]: inside [R_total][text_cap][H] only while
    // text_avail <= text_cap
    if (text_rows && text_avail && text_cap > 0)
        for (int r = row0; r < row0 + R; r++)
            if (text_avail[r] < 0 || text_avail[r] > text_cap) return -2;
    const size_t rt = (size_t)R_total, nc = (size_t)frame_cap * rt * 16;
    const int Rp = (R_total + 15) / 16 * 16;   // fragment order: blocks of 16 rows
    DBuf dl, dcodes, dnf, dforced, dseed, dslots, dtab, dqkv, dgam, dtemb, dcpt, dcptp, dpad, dh, dssq, dxh, dqo, dtrows, dtav, dheld, drules, dscores;
    if (scores && !dscores.up(scores, nc * 4)) return -1000;
    if (rules && !drules.up(rules, rt * sizeof(SlotRules))) return -1000;
    if (text_rows && !dtrows.up(text_rows, rt * (size_t)(text_cap > 0 ? text_cap : 1) * (H > 0 ? H : 1) * 4)) return -1000;
    if (text_avail && !dtav.up(text_avail, rt * 4)) return -1000;
    if (held && !dheld.up(held, rt * 4)) return -1000;
    if (!dl.up(logits, rt * V * 4) || !dcodes.up(codes, nc * 4) || !dnf.up(n_frames, rt * 4)) return -1000;
    if (forced && !dforced.up(forced, nc * 4)) return -1000;
    if (seed_ptr && !dseed.up(seed_ptr, rt * 8)) return -1000;
    if (slots && !dslots.up(slots, rt * sizeof(SlotParams))) return -1000;
    CpArgmaxArgs a;
    a.logits = (const float*)dl.p;
    a.V = V;
    a.R = R;
    a.H = H;
    a.row0 = row0;
    a.R_total = R_total;
    a.group = group;
    a.codes = (int*)dcodes.p;
    a.n_frames = (const int*)dnf.p;
    a.frame_cap = frame_cap;
    a.temperature = temperature;
    a.top_k = top_k;
    a.seed = seed;
    a.seed_ptr = seed_ptr ? (const unsigned long long*)dseed.p : nullptr;
    a.forced = forced ? (const int*)dforced.p : nullptr;
    a.slots = slots ? (const SlotParams*)dslots.p : nullptr;
    a.text_rows = text_rows ? (const float*)dtrows.p : nullptr;
    a.text_avail = text_avail ? (const int*)dtav.p : nullptr;
    a.text_cap = text_cap;
    a.held = held ? (const int*)dheld.p : nullptr;
    a.rules = rules ? (const SlotRules*)drules.p : nullptr;
    a.scores = scores ? (float*)dscores.p : nullptr;
    std::vector<float> hh;
    std::vector<uint16_t> hx;
    if (epilogue) {
        hh.assign((size_t)Rp * H, 0.f);
        for (int r = 0; r < R_total; r++)
            for (int k = 0; k < H; k++) hh[frag_idx(r, k, H)] = h_out[(size_t)r * H + k];
        if (!dh.up(hh.data(), hh.size() * 4) || !dssq.up(ssq_out, rt * (H / 16) * 4)) return -1000;
        a.h_out = (float*)dh.p;
        a.ssq_out = (float*)dssq.p;
        if (xh_out) {
            hx.assign((size_t)Rp * H, 0);
            for (int r = 0; r < R_total; r++)
                for (int k = 0; k < H; k++) hx[frag_idx(r, k, H)] = xh_out[(size_t)r * H + k];
            if (!dxh.up(hx.data(), hx.size() * 2) || !dgam.up(gamma, (size_t)H * 4)) return -1000;
            a.xh_out = (half_t*)dxh.p;
            a.gamma_next = (const float*)dgam.p;
        }
    }
    if (epilogue == 1) {
        if (!dtab.up(next_table, (size_t)V * H * 4)) return -1000;
        a.next_table = (const float*)dtab.p;
        if (next_qkv) {
            if (!dqkv.up(next_qkv, (size_t)V * qkv_ld * 4) || !dqo.up(qkv_out, rt * qkv_ld * 4)) return -1000;
            a.next_qkv = (const float*)dqkv.p;
            a.qkv_out = (float*)dqo.p;
            a.qkv_ld = qkv_ld;
        }
    } else if (epilogue == 2) {
        const size_t tab = (size_t)V * H;
        if (!dtemb.up(talker_emb, (size_t)talker_vocab * H * 4) || !dcpt.up(cp_tables, (size_t)n_groups * tab * 4)) return -1000;
        std::vector<const float*> ptrs(n_groups);
        for (int g = 0; g < n_groups; g++) ptrs[g] = (const float*)dcpt.p + (size_t)g * tab;
        if (!dcptp.up(ptrs.data(), ptrs.size() * sizeof(const float*))) return -1000;
        if (pad && !dpad.up(pad, (size_t)H * 4)) return -1000;
        a.talker_emb = (const float*)dtemb.p;
        a.talker_vocab = talker_vocab;
        a.cp_tables = (const float* const*)dcptp.p;
        a.n_groups = n_groups;
        a.pad_embed = pad ? (const float*)dpad.p : nullptr;
    }
    if (const int rc = launch_cp_argmax(nullptr, a)) return rc;
    Q3_HIP(hipDeviceSynchronize(), -1000);
    Q3_HIP(hipMemcpy(codes, dcodes.p, nc * 4, hipMemcpyDeviceToHost), -1000);
    if (scores) Q3_HIP(hipMemcpy(scores, dscores.p, nc * 4, hipMemcpyDeviceToHost), -1000);
    if (epilogue) {
        Q3_HIP(hipMemcpy(hh.data(), dh.p, hh.size() * 4, hipMemcpyDeviceToHost), -1000);
        for (int r = 0; r < R_total; r++)
            for (int k = 0; k < H; k++) h_out[(size_t)r * H + k] = hh[frag_idx(r, k, H)];
        Q3_HIP(hipMemcpy(ssq_out, dssq.p, rt * (H / 16) * 4, hipMemcpyDeviceToHost), -1000);
        if (xh_out) {
            Q3_HIP(hipMemcpy(hx.data(), dxh.p, hx.size() * 2, hipMemcpyDeviceToHost), -1000);
            for (int r = 0; r < R_total; r++)
                for (int k = 0; k < H; k++) xh_out[(size_t)r * H + k] = hx[frag_idx(r, k, H)];
        }
        if (a.qkv_out) Q3_HIP(hipMemcpy(qkv_out, dqo.p, rt * qkv_ld * 4, hipMemcpyDeviceToHost), -1000);
    }
    return 0;
}
extern "C" int q3t_cp_sample_case(const float* logits, int V, int R_total, int row0, int R, int group, int* codes,
                                  const int* n_frames, int frame_cap, const int* forced, float temperature, int top_k,
                                  unsigned long long seed, const unsigned long long* seed_ptr, const void* slots,
                                  int epilogue, int H, const float* next_table, const float* next_qkv, int qkv_ld,
                                  const float* gamma, const float* talker_emb, int talker_vocab, const float* cp_tables,
                                  int n_groups, const float* pad, float* h_out, float* ssq_out, uint16_t* xh_out,
                                  float* qkv_out) {
    return cp_sample_case(logits, V, R_total, row0, R, group, codes, n_frames, frame_cap, forced, temperature, top_k, seed,
                          seed_ptr, slots, epilogue, H, next_table, next_qkv, qkv_ld, gamma, talker_emb, talker_vocab, cp_tables,
                          n_groups, pad, h_out, ssq_out, xh_out, qkv_out, nullptr, nullptr, 0, nullptr);
}
// q3t_cp_sample_case with streamed text and held rows (CpArgmaxArgs): text_rows[R_total][max(text_cap, 1)][H],
// text_avail[R_total] (<= text_cap on the rows of the launch, else -2), held[R_total]; each may be null.
extern "C" int q3t_cp_sample_text_case(const float* logits, int V, int R_total, int row0, int R, int group, int* codes,
                                       const int* n_frames, int frame_cap, const int* forced, float temperature, int top_k,
                                       unsigned long long seed, const unsigned long long* seed_ptr, const void* slots,
                                       int epilogue, int H, const float* next_table, const float* next_qkv, int qkv_ld,
                                       const float* gamma, const float* talker_emb, int talker_vocab, const float* cp_tables,
                                       int n_groups, const float* pad, float* h_out, float* ssq_out, uint16_t* xh_out,
                                       float* qkv_out, const float* text_rows, const int* text_avail, int text_cap,
                                       const int* held) {
    return cp_sample_case(logits, V, R_total, row0, R, group, codes, n_frames, frame_cap, forced, temperature, top_k, seed,
                          seed_ptr, slots, epilogue, H, next_table, next_qkv, qkv_ld, gamma, talker_emb, talker_vocab, cp_tables,
                          n_groups, pad, h_out, ssq_out, xh_out, qkv_out, text_rows, text_avail, text_cap, held);
}
// q3t_cp_sample_text_case with sampler rules (CpArgmaxArgs::rules): rules = SlotRules[R_total], or null.
extern "C" int q3t_cp_sample_rules_case(const float* logits, int V, int R_total, int row0, int R, int group, int* codes,
                                        const int* n_frames, int frame_cap, const int* forced, float temperature, int top_k,
                                        unsigned long long seed, const unsigned long long* seed_ptr, const void* slots,
                                        int epilogue, int H, const float* next_table, const float* next_qkv, int qkv_ld,
                                        const float* gamma, const float* talker_emb, int talker_vocab, const float* cp_tables,
                                        int n_groups, const float* pad, float* h_out, float* ssq_out, uint16_t* xh_out,
                                        float* qkv_out, const float* text_rows, const int* text_avail, int text_cap,
                                        const int* held, const void* rules) {
    return cp_sample_case(logits, V, R_total, row0, R, group, codes, n_frames, frame_cap, forced, temperature, top_k, seed,
                          seed_ptr, slots, epilogue, H, next_table, next_qkv, qkv_ld, gamma, talker_emb, talker_vocab, cp_tables,
                          n_groups, pad, h_out, ssq_out, xh_out, qkv_out, text_rows, text_avail, text_cap, held, rules);
}
// q3t_cp_sample_rules_case with the log-probability of the id the stream continues with (CpArgmaxArgs::scores):
// scores[frame_cap][R_total][16] in and out, whole.  Null: q3t_cp_sample_rules_case itself.
extern "C" int q3t_cp_score_case(const float* logits, int V, int R_total, int row0, int R, int group, int* codes,
                                 const int* n_frames, int frame_cap, const int* forced, float temperature, int top_k,
                                 unsigned long long seed, const unsigned long long* seed_ptr, const void* slots,
                                 int epilogue, int H, const float* next_table, const float* next_qkv, int qkv_ld,
                                 const float* gamma, const float* talker_emb, int talker_vocab, const float* cp_tables,
                                 int n_groups, const float* pad, float* h_out, float* ssq_out, uint16_t* xh_out,
                                 float* qkv_out, const float* text_rows, const int* text_avail, int text_cap,
                                 const int* held, const void* rules, float* scores) {
    return cp_sample_case(logits, V, R_total, row0, R, group, codes, n_frames, frame_cap, forced, temperature, top_k, seed,
                          seed_ptr, slots, epilogue, H, next_table, next_qkv, qkv_ld, gamma, talker_emb, talker_vocab, cp_tables,
                          n_groups, pad, h_out, ssq_out, xh_out, qkv_out, text_rows, text_avail, text_cap, held, rules, scores);
}

// ---- launch-boundary microbenchmark: a dependent chain of n small kernels, captured as a graph ----
namespace {
__global__ void chain_empty_kernel(float* buf) { (void)buf; }
// every thread reads what the previous kernel wrote (another workgroup's element) and writes its own
__global__ void chain_dep_kernel(const float* __restrict__ in, float* __restrict__ out, int n, int hops) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    int j = (i * 97 + 13) % n;
    float v = in[j];
    for (int h = 1; h < hops; h++) {  // extra dependent round trips
        j = ((int)(v * 0.f) + j * 31 + 7) % n;
        v += in[j];
    }
    out[i] = v + 1.0f;
}
}  // namespace

// kind 0: empty kernels; kind >=1: `kind` dependent global round trips per kernel.
// Returns average microseconds per kernel over `iters` graph replays of an n-kernel chain.
extern "C" float q3t_bench_chain(int kind, int blocks, int threads, int n_kernels, int iters, int use_graph) {
    hipStream_t s = nullptr;
    if (hipStreamCreate(&s) != hipSuccess) return -1.f;
    const int n = blocks * threads;
    DBuf a, b;
    if (!a.alloc((size_t)n * 4) || !b.alloc((size_t)n * 4)) return -1.f;
    hipMemset(a.p, 0, (size_t)n * 4);
    hipMemset(b.p, 0, (size_t)n * 4);
    auto chain = [&]() {
        for (int k = 0; k < n_kernels; k++) {
            float* in = (float*)((k & 1) ? b.p : a.p);
            float* out = (float*)((k & 1) ? a.p : b.p);
            if (kind == 0) hipLaunchKernelGGL(chain_empty_kernel, dim3(blocks), dim3(threads), 0, s, out);
            else hipLaunchKernelGGL(chain_dep_kernel, dim3(blocks), dim3(threads), 0, s, in, out, n, kind);
        }
    };
    hipGraph_t g = nullptr;
    hipGraphExec_t ge = nullptr;
    chain();
    hipStreamSynchronize(s);
    if (use_graph) {
        hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed);
        chain();
        if (hipStreamEndCapture(s, &g) != hipSuccess) return -1.f;
        if (hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) != hipSuccess) return -1.f;
        hipGraphLaunch(ge, s);
        hipStreamSynchronize(s);
    }
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    hipEventRecord(e0, s);
    for (int it = 0; it < iters; it++) {
        if (use_graph) hipGraphLaunch(ge, s);
        else chain();
    }
    hipEventRecord(e1, s);
    hipStreamSynchronize(s);
    float ms = 0.f;
    hipEventElapsedTime(&ms, e0, e1);
    if (ge) hipGraphExecDestroy(ge);
    if (g) hipGraphDestroy(g);
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    hipStreamDestroy(s);
    return ms * 1000.f / ((float)iters * n_kernels);
}

// ---- CPU-side hook: parse weight files the way the loaders do (container, or the reference's .npz /
// .npy / .safetensors natively) and report what was found.  No GPU call.  Writes up to `cap` bytes of
// "name dtype ndim d0 d1 d2 d3 fnv1a64-of-bytes\n" lines; returns the tensor count or -1.
extern "C" int q3t_inspect_weights(const char* path, const char* aux_dir, char* out, int cap) {
    Pack p;
    if (!p.open_auto(path, aux_dir)) return -1;
    std::string s;
    for (const auto& kv : p.tensors) {
        const PackTensor& t = kv.second;
        unsigned long long h = 1469598103934665603ull;
        for (uint64_t i = 0; i < t.nbytes; i++) h = (h ^ t.data[i]) * 1099511628211ull;
        char line[256];
        snprintf(line, sizeof(line), "%s %u %u %llu %llu %llu %llu %llx\n", t.name.c_str(), t.dtype, t.ndim,
                 (unsigned long long)t.shape[0], (unsigned long long)t.shape[1], (unsigned long long)t.shape[2],
                 (unsigned long long)t.shape[3], h);
        s += line;
    }
    for (const auto& kv : p.meta) {
        char line[128];
        snprintf(line, sizeof(line), "meta %s %.17g\n", kv.first.c_str(), kv.second);
        s += line;
    }
    if (out && cap > 0) {
        const size_t n = s.size() < (size_t)cap - 1 ? s.size() : (size_t)cap - 1;
        memcpy(out, s.data(), n);
        out[n] = 0;
    }
    return (int)p.tensors.size();
}

// ---- the code predictor's layer-0 q|k|v table (Model::cp_qkv_tab) against the launch it replaces ----
// A model with the code-predictor stack (and whatever Q3_CP_QKV_TABLE made of the table); null on failure.
extern "C" void* q3t_cp_model_load(const char* path) { return model_load(path, false, true); }
extern "C" void q3t_cp_model_free(void* m) { model_free((Model*)m); }
// q|k|v columns of a row; 0 when the model carries no table
extern "C" int q3t_cp_qkv_ld(void* mm) {
    const Model* m = (const Model*)mm;
    return m && m->cp_qkv_tab ? (m->cfg.n_heads + 2 * m->cfg.n_kv) * m->cfg.head_dim : 0;
}
// 1 when a code-predictor pass of `rows` rows takes layer 0's q|k|v from the table (cp_frame's own predicate)
extern "C" int q3t_cp_qkv_serves(void* mm, int rows) { return mm && ((const Model*)mm)->cp_qkv_serves(rows) ? 1 : 0; }
// out[i][ld] = table row toks[i] of `group` (the tokens of cp.codec_emb.<group>); ids outside the vocabulary: -2
extern "C" int q3t_cp_qkv_tab(void* mm, int group, const int* toks, int n, float* out) {
    const Model* m = (const Model*)mm;
    const int ld = q3t_cp_qkv_ld(mm);
    if (!ld || group < 0 || group + 1 >= m->cfg.cp_groups) return -1;
    for (int i = 0; i < n; i++) {
        if (toks[i] < 0 || toks[i] >= m->cfg.cp_vocab) return -2;
        Q3_HIP(hipMemcpy(out + (size_t)i * ld, m->cp_qkv_rows(group) + (size_t)toks[i] * ld, (size_t)ld * 4, hipMemcpyDeviceToHost), -1);
    }
    return 0;
}
// The live launch at R rows: the embedding gather of rows toks[0..R) of cp.codec_emb.<group> into a pass's workspace
// (h, ssq partials, xh), then run_stack's layer-0 q|k|v launch over rows [row0, row0 + R); out[R][ld].  The variant the
// launch took is in q3t_last_linear_variant().
extern "C" int q3t_cp_qkv_live(void* mm, int group, const int* toks, int R, int row0, float* out) {
    const Model* m = (const Model*)mm;
    if (!m || !m->has_cp || group < 0 || group >= m->cfg.cp_groups || R <= 0 || row0 % 16) return -1;
    const ModelCfg& c = m->cfg;
    const int H = c.hidden, ld = (c.n_heads + 2 * c.n_kv) * c.head_dim;
    Work w;
    DBuf dt;
    std::vector<int> tk((size_t)row0 + R, -1);
    for (int i = 0; i < R; i++) tk[row0 + i] = toks[i];
    int rc = -1;
    if (work_alloc(w, c, row0 + R, c.cp_ffn, c.cp_vocab) == 0 && dt.up(tk.data(), tk.size() * 4) &&
        work_zero(nullptr, w, c, c.cp_ffn, c.cp_vocab) == 0 &&
        launch_gather_embed(nullptr, m->cp_emb[group], c.cp_vocab, H, (const int*)dt.p, 1, nullptr, 0, 0, w.h, w.ssq, R, row0, 0,
                            nullptr, w.xh, m->cp.L[0].in_ln) == 0) {
        LinArgs a;   // as run_stack builds it
        a.wp = m->cp.L[0].qkv.wp;
        a.N = m->cp.L[0].qkv.N;
        a.K = H;
        a.M = row0 + R;
        a.m_begin = row0;
        a.nt = m->cp.nt;
        a.x16 = w.xh;
        a.ssq = w.ssq;
        a.ssq_parts = H / 16;
        a.eps = c.eps;
        a.y = w.qkv;
        a.ldy = ld;
        if (launch_linear(nullptr, a, PRO_NORM, EPI_STORE) == 0 && hipDeviceSynchronize() == hipSuccess &&
            hipMemcpy(out, w.qkv + (size_t)row0 * ld, (size_t)R * ld * 4, hipMemcpyDeviceToHost) == hipSuccess)
            rc = 0;
    }
    work_free(w);
    return rc;
}

// ---- streaming encode (enc_stream_*, csrc/q3_enc_stream.hip) ----
// enc_stream_push that also hands back the pre-quantiser embedding columns of the push: emb [frames][*channels], packed like
// the codes (emb must hold the push's frames x the encoder's hidden width).
extern "C" int q3t_enc_stream_embeddings(void* s, int n, const int32_t* streams, const float* pcm, const int32_t* n_new,
                                         const int32_t* finish, int64_t* codes_out, int64_t out_capacity_frames, int64_t* offsets,
                                         float* emb, int* channels) {
    if (!emb || !channels) return -1;
    return enc_stream_push_impl((EncStream*)s, n, streams, pcm, n_new, finish, codes_out, out_capacity_frames, offsets, emb, channels);
}
// The host arithmetic of a push, no device call: a stream of `before` samples takes n_new more (and finishes) -> n_in
// [n_levels + 1] new columns per level (the last: frames handed out), before_cols [n_levels + 1], carry [n_levels] columns
// each strided op holds when the push starts.
extern "C" int q3t_enc_stream_plan(const int* ks, const int* strides, int n_levels, long long before, long long n_new, int finish,
                                   long long* n_in, long long* before_cols, long long* carry) {
    if (!ks || !strides || n_levels < 1 || before < 0 || n_new < 0) return -1;
    enc_stream_plan(ks, strides, n_levels, before, n_new, finish != 0, n_in, before_cols, carry);
    return 0;
}

// ---- the encoder's own kernels (csrc/q3_enc.hip), one launch each ----
extern "C" int q3t_enc_rvq_tile(int n_frames) { return enc_rvq_tile(n_frames); }

// One enc_launch_rvq over the tables enc_load builds (enc_rvq_tables) from codebook [nq][cb][dim].  stream == 0, the clip
// layout of enc_run: z [B][2 * dim][T] in, on the device rows of pitch enc_pitch(T) whose pad columns hold NaN, frame
// g = b * T + t.  stream != 0, the layout of an EncStream push: z [B][2 * dim] (B frames), ld = T = 1.  -> codes [B * T][nq].
// -2: a geometry enc_load refuses (or a non-finite codebook), before anything launches; -3: the launch wrote outside
// codes [0, B * T * nq) (the device buffer is one 16-frame tile longer and filled with a sentinel); -1: a HIP error.
extern "C" int q3t_enc_rvq_case(const float* codebook, int nq, int cb, int dim, int n_sem, int stream, int B, int T, const float* z,
                                int64_t* codes) {
    constexpr int64_t GUARD = 0x5a5a5a5a5a5a5a5aLL;
    if (!codebook || !z || !codes || !enc_rvq_geometry(nq, cb, dim, n_sem)) return -2;
    if (B < 1 || T < 1 || (stream && T != 1) || (long long)B * T > (1 << 24)) return -2;
    const size_t ne = (size_t)nq * cb * dim;
    for (size_t i = 0; i < ne; i++)
        if (!std::isfinite(codebook[i])) return -2;
    const int n_frames = B * T, ld = stream ? 1 : (int)enc_pitch(T);
    const size_t rows = (size_t)B * 2 * dim;
    std::vector<float> hz(rows * ld, std::nanf(""));
    for (size_t r = 0; r < rows; r++) memcpy(hz.data() + r * ld, z + r * T, (size_t)T * 4);
    std::vector<int64_t> hc((size_t)(n_frames + 16) * nq, GUARD);
    DeviceAllocs mem;
    EncOp op;
    op.op = EOP_RVQ;
    op.cin = 2 * dim;
    op.nq = nq;
    op.cb = cb;
    op.dim = dim;
    op.n_sem = n_sem;
    if (!enc_rvq_tables(mem, codebook, op)) return -1;
    DBuf dz, dc;
    if (!dz.up(hz.data(), hz.size() * 4) || !dc.up(hc.data(), hc.size() * 8)) return -1;
    Q3_HIP(hipDeviceSynchronize(), -1);
    if (enc_launch_rvq(nullptr, (const float*)dz.p, ld, T, n_frames, op, (int64_t*)dc.p)) return -1;
    Q3_HIP(hipDeviceSynchronize(), -1);
    Q3_HIP(hipMemcpy(hc.data(), dc.p, hc.size() * 8, hipMemcpyDeviceToHost), -1);
    memcpy(codes, hc.data(), (size_t)n_frames * nq * 8);
    for (size_t i = (size_t)n_frames * nq; i < hc.size(); i++)
        if (hc[i] != GUARD) return -3;
    return 0;
}

// One enc_launch_conv_in: x [B][n] (device rows of pitch enc_pitch(n), NaN in the pad), w [cout][k], bias [cout] or null
// -> y [B][cout][n].  hist == null: whole clips.  Else entry b continues stream streams[b] (distinct, < max_streams) of
// hist [max_streams][k - 1], which comes back as the call left it.  -2: arguments the encoder never passes; -3: a pad column
// of y or a word behind the history block was written; -1: a HIP error.
extern "C" int q3t_enc_conv_in_case(const float* x, int B, int n, const float* w, const float* bias, int cout, int k, float* hist,
                                    int max_streams, const int* streams, float* y) {
    constexpr uint32_t GUARD = 0x7fc5a5a5u;   // a NaN pattern the kernel never produces
    if (!x || !w || !y || B < 1 || n < 1 || cout < 1 || k < 1 || k > ENC_IN_MAXK) return -2;
    if ((hist != nullptr) != (streams != nullptr)) return -2;
    const int H = k - 1;
    if (hist) {
        if (max_streams < B) return -2;
        std::vector<char> seen((size_t)max_streams, 0);
        for (int b = 0; b < B; b++)
            if (streams[b] < 0 || streams[b] >= max_streams || seen[(size_t)streams[b]]++) return -2;
    }
    const int ld = (int)enc_pitch(n);
    std::vector<float> hx((size_t)B * ld, std::nanf(""));
    for (int b = 0; b < B; b++) memcpy(hx.data() + (size_t)b * ld, x + (size_t)b * n, (size_t)n * 4);
    const size_t ny = (size_t)B * cout;
    std::vector<uint32_t> hy(ny * ld, GUARD);
    const size_t nh = hist ? (size_t)max_streams * H : 0;
    std::vector<uint32_t> hh(nh + 32, GUARD);
    if (nh) memcpy(hh.data(), hist, nh * 4);
    DBuf dx, dw, db, dy, dh, ds;
    if (!dx.up(hx.data(), hx.size() * 4) || !dw.up(w, (size_t)cout * k * 4) || !dy.up(hy.data(), hy.size() * 4) ||
        !dh.up(hh.data(), hh.size() * 4))
        return -1;
    if (bias && !db.up(bias, (size_t)cout * 4)) return -1;
    if (hist && !ds.up(streams, (size_t)B * 4)) return -1;
    EncOp op;
    op.op = EOP_CONV_IN;
    op.cin = 1;
    op.cout = cout;
    op.k = k;
    op.w = (float*)dw.p;
    op.bias = bias ? (float*)db.p : nullptr;
    Q3_HIP(hipDeviceSynchronize(), -1);
    if (enc_launch_conv_in(nullptr, (const float*)dx.p, ld, op, (float*)dy.p, ld, n, B, hist ? (float*)dh.p : nullptr, H,
                           hist ? (const int*)ds.p : nullptr))
        return -1;
    Q3_HIP(hipDeviceSynchronize(), -1);
    Q3_HIP(hipMemcpy(hy.data(), dy.p, hy.size() * 4, hipMemcpyDeviceToHost), -1);
    Q3_HIP(hipMemcpy(hh.data(), dh.p, hh.size() * 4, hipMemcpyDeviceToHost), -1);
    int outside = 0;
    for (size_t r = 0; r < ny; r++) {
        memcpy(y + r * n, hy.data() + r * ld, (size_t)n * 4);
        for (int l = n; l < ld; l++) outside += hy[r * ld + l] != GUARD;
    }
    if (nh) memcpy(hist, hh.data(), nh * 4);
    for (size_t i = nh; i < hh.size(); i++) outside += hh[i] != GUARD;
    return outside ? -3 : 0;
}

// ---- the frame loop's row kernels, one launch each (tests/test_gpu_row_kernels.py) ----------------------------------
namespace {
constexpr uint32_t ROW_GUARD32 = 0x7fc5a5a5u;   // the NaN patterns of q3t_linear_case
constexpr uint16_t ROW_GUARD16 = 0x7d5au;

// What a producer of residual rows writes -- h (f32, fragment order or row-major), ssq partials [row][H/16], xh (fp16,
// fragment order) -- each over its 16-row-padded extent and filled with guards before the launch.
struct RowOut {
    int Rp = 0, H = 0, parts = 0;
    bool frag = true;
    std::vector<uint32_t> h, s;
    std::vector<uint16_t> x;
    DBuf dh, ds, dx;
    bool init(int rows, int H_, bool with_h, bool with_s, bool with_x, bool frag_ = true) {
        Rp = (rows + 15) / 16 * 16;
        H = H_;
        parts = H / 16;
        frag = frag_;
        if (with_h) h.assign((size_t)Rp * H, ROW_GUARD32);
        if (with_s) s.assign((size_t)Rp * parts, ROW_GUARD32);
        if (with_x) x.assign((size_t)Rp * H, ROW_GUARD16);
        return (!with_h || dh.up(h.data(), h.size() * 4)) && (!with_s || ds.up(s.data(), s.size() * 4)) &&
               (!with_x || dx.up(x.data(), x.size() * 2));
    }
    float* ph() { return h.empty() ? nullptr : (float*)dh.p; }
    float* ps() { return s.empty() ? nullptr : (float*)ds.p; }
    half_t* px() { return x.empty() ? nullptr : (half_t*)dx.p; }
    size_t at(int r, int k) const { return frag ? frag_idx(r, k, H) : (size_t)r * H + k; }
    // Rows own(r) go to the host arrays (row-major, rows of the caller's own count); -> the number of words of every other
    // row that no longer hold their guard, or -1 on a HIP error.
    template <class F>
    int collect(F own, float* h_out, float* ssq_out, uint16_t* xh_out) {
        if (!h.empty() && hipMemcpy(h.data(), dh.p, h.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
        if (!s.empty() && hipMemcpy(s.data(), ds.p, s.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
        if (!x.empty() && hipMemcpy(x.data(), dx.p, x.size() * 2, hipMemcpyDeviceToHost) != hipSuccess) return -1;
        int outside = 0;
        for (int r = 0; r < Rp; r++) {
            const bool mine = own(r);
            for (int k = 0; k < H; k++) {
                const size_t i = at(r, k);
                if (mine) {
                    if (!h.empty()) memcpy(&h_out[(size_t)r * H + k], &h[i], 4);
                    if (!x.empty()) xh_out[(size_t)r * H + k] = x[frag_idx(r, k, H)];
                } else {
                    if (!h.empty() && h[i] != ROW_GUARD32) outside++;
                    if (!x.empty() && x[frag_idx(r, k, H)] != ROW_GUARD16) outside++;
                }
            }
            if (!s.empty())
                for (int p = 0; p < parts; p++) {
                    const uint32_t v = s[(size_t)r * parts + p];
                    if (mine) memcpy(&ssq_out[(size_t)r * parts + p], &v, 4);
                    else if (v != ROW_GUARD32) outside++;
                }
        }
        return outside;
    }
};

// cp_tables[n_tab][cp_vocab][H] (one contiguous host array) -> the device array of 16 table pointers the kernels index
// with the group (entries beyond n_tab repeat the last table, so that no group index leaves the array)
bool upload_tables(const float* cp_tables, int n_tab, int cp_vocab, int H, DBuf& dtab, DBuf& dptrs) {
    const size_t tab = (size_t)cp_vocab * H;
    if (!dtab.up(cp_tables, (size_t)n_tab * tab * 4)) return false;
    const float* ptrs[16];
    for (int g = 0; g < 16; g++) ptrs[g] = (const float*)dtab.p + (size_t)(g < n_tab ? g : n_tab - 1) * tab;
    return dptrs.up(ptrs, sizeof(ptrs));
}
}  // namespace

// One launch_final_norm over output rows row0 .. row0+R-1 of `rows`-row buffers.  h[rows][H] and ssq[rows][parts] are
// row-major on the host (h is laid out in fragment order here; padding rows hold finite poison); the source row of output
// row r is row_map[r] (row_map[rows], indexed by the output row) or, with row_map null, r + src_off.  want_f32 / want_f16 /
// want_copy say which outputs the launch produces: out_f32[rows][H], out_f16[rows][H] (fp16 bits), and out_copy[rows][H]
// with out_copy_ssq[rows][H/16] and -- with out_copy_gamma[H] -- out_copy_xh[rows][H], whose row r + out_copy_row_off is
// the copy of output row r.  Every output is a guard pattern over its 16-row-padded extent before the launch; the rows the
// launch owns come back (row-major), the others stay as the caller passed them.  -3: anything outside those rows changed;
// -2: arguments no caller passes (a source or copy row outside the buffers, parts != H / 16, a wanted output without its
// array, out_copy_xh without out_copy_gamma or the reverse); -1: the launcher's refusal or a HIP error.
extern "C" int q3t_final_norm_case(const float* h, const float* ssq, int rows, int H, int parts, const float* gamma, float eps,
                                   int R, int row0, const int* row_map, int src_off, int want_f32, int want_f16, int want_copy,
                                   int out_copy_row_off, const float* out_copy_gamma, float* out_f32, uint16_t* out_f16,
                                   float* out_copy, float* out_copy_ssq, uint16_t* out_copy_xh) {
    if (!h || !ssq || !gamma || rows <= 0 || H <= 0 || H % 32 || parts != H / 16 || R <= 0 || row0 < 0 || row0 + R > rows) return -2;
    if ((want_f32 && !out_f32) || (want_f16 && !out_f16) || (want_copy && (!out_copy || !out_copy_ssq))) return -2;
    if ((out_copy_xh != nullptr) != (out_copy_gamma != nullptr) || (out_copy_xh && !want_copy)) return -2;
    if (want_copy && (row0 + out_copy_row_off < 0 || row0 + R + out_copy_row_off > rows)) return -2;
    for (int r = row0; r < row0 + R; r++) {
        const int src = row_map ? row_map[r] : r + src_off;
        if (src < 0 || src >= rows) return -2;
    }
    const int Rp = (rows + 15) / 16 * 16;
    std::vector<float> hp((size_t)Rp * H, 3.0e4f), sp((size_t)Rp * parts, 1.0e9f);
    for (int r = 0; r < rows; r++) {
        for (int k = 0; k < H; k++) hp[frag_idx(r, k, H)] = h[(size_t)r * H + k];
        memcpy(&sp[(size_t)r * parts], &ssq[(size_t)r * parts], (size_t)parts * 4);
    }
    DBuf dh, ds, dg, dmap, dcg;
    if (!dh.up(hp.data(), hp.size() * 4) || !ds.up(sp.data(), sp.size() * 4) || !dg.up(gamma, (size_t)H * 4)) return -1;
    if (row_map && !dmap.up(row_map, (size_t)rows * 4)) return -1;
    if (out_copy_gamma && !dcg.up(out_copy_gamma, (size_t)H * 4)) return -1;
    RowOut o32, o16, oc;
    if (!o32.init(rows, H, want_f32, false, false, false) || !o16.init(rows, H, false, false, want_f16) ||
        !oc.init(rows, H, want_copy, want_copy, want_copy && out_copy_xh))
        return -1;
    FinalNormArgs a;
    a.h = (const float*)dh.p;
    a.ssq = (const float*)ds.p;
    a.ssq_parts = parts;
    a.gamma = (const float*)dg.p;
    a.eps = eps;
    a.R = R;
    a.H = H;
    a.row0 = row0;
    a.row_map = row_map ? (const int*)dmap.p : nullptr;
    a.src_off = src_off;
    a.out_f32 = o32.ph();
    a.out_f16 = o16.px();
    a.out_copy = oc.ph();
    a.out_copy_ssq = oc.ps();
    a.out_copy_row_off = out_copy_row_off;
    a.out_copy_xh = oc.px();
    a.out_copy_gamma = out_copy_gamma ? (const float*)dcg.p : nullptr;
    Q3_HIP(hipDeviceSynchronize(), -1);
    if (launch_final_norm(nullptr, a)) return -1;
    Q3_HIP(hipDeviceSynchronize(), -1);
    auto own = [&](int r) { return r >= row0 && r < row0 + R; };
    auto own_copy = [&](int r) { return r >= row0 + out_copy_row_off && r < row0 + R + out_copy_row_off; };
    const int c32 = o32.collect(own, out_f32, nullptr, nullptr), c16 = o16.collect(own, nullptr, nullptr, out_f16);
    const int cc = oc.collect(own_copy, out_copy, out_copy_ssq, out_copy_xh);
    if (c32 < 0 || c16 < 0 || cc < 0) return -1;
    return (c32 || c16 || cc) ? -3 : 0;
}

// One launch_gather_embed over rows row0 .. row0+R-1 of R_total.  n_frames null: the `tok` form, tok[R_total * tok_stride]
// (row r reads tok[r * tok_stride]).  n_frames[R_total] given: the `codes` form, tok = codes[frame_cap][R_total][16], column
// col of the row's current frame, forced (same layout) or null.  h[R_total][H], ssq[R_total][H/16] and, with gamma[H],
// xh[R_total][H] come back row-major for the rows of the launch; guards and return codes as q3t_final_norm_case.
extern "C" int q3t_gather_embed_case(const float* table, int V, int H, const int* tok, int tok_stride, const int* n_frames,
                                     int frame_cap, int col, const int* forced, int R, int row0, int R_total,
                                     const float* gamma, float* h, float* ssq, uint16_t* xh) {
    if (!table || V <= 0 || H <= 0 || H % 32 || !tok || R <= 0 || row0 < 0 || row0 + R > R_total || !h || !ssq) return -2;
    if ((xh != nullptr) != (gamma != nullptr)) return -2;
    if (n_frames ? (frame_cap < 1 || col < 0 || col > 15) : (tok_stride < 1 || forced)) return -2;
    const size_t nt = n_frames ? (size_t)frame_cap * R_total * 16 : (size_t)R_total * tok_stride;
    DBuf dt, dtok, dnf, dfz, dg;
    if (!dt.up(table, (size_t)V * H * 4) || !dtok.up(tok, nt * 4)) return -1;
    if (n_frames && !dnf.up(n_frames, (size_t)R_total * 4)) return -1;
    if (forced && !dfz.up(forced, nt * 4)) return -1;
    if (gamma && !dg.up(gamma, (size_t)H * 4)) return -1;
    RowOut o;
    if (!o.init(R_total, H, true, true, xh != nullptr)) return -1;
    Q3_HIP(hipDeviceSynchronize(), -1);
    if (launch_gather_embed(nullptr, (const float*)dt.p, V, H, (const int*)dtok.p, tok_stride, n_frames ? (const int*)dnf.p : nullptr,
                            frame_cap, col, o.ph(), o.ps(), R, row0, R_total, forced ? (const int*)dfz.p : nullptr, o.px(),
                            gamma ? (const float*)dg.p : nullptr))
        return -1;
    Q3_HIP(hipDeviceSynchronize(), -1);
    const int c = o.collect([&](int r) { return r >= row0 && r < row0 + R; }, h, ssq, xh);
    return c < 0 ? -1 : c ? -3 : 0;
}

// One launch_feedback over R rows: codes16[R][16], talker_emb[talker_vocab][H], cp_tables[n_groups][cp_vocab][H] (one
// contiguous array), pad[H] or null.  h[R][H], ssq[R][H/16] and, with gamma[H], xh[R][H] come back; guards (the rows that pad
// R to 16) and return codes as q3t_final_norm_case.
extern "C" int q3t_feedback_case(const int* codes16, int R, const float* talker_emb, int talker_vocab, const float* cp_tables,
                                 int cp_vocab, int n_groups, const float* pad, int H, const float* gamma, float* h, float* ssq,
                                 uint16_t* xh) {
    if (!codes16 || R <= 0 || !talker_emb || talker_vocab <= 0 || !cp_tables || cp_vocab <= 0 || n_groups < 1 || n_groups > 15 ||
        H <= 0 || H % 32 || !h || !ssq || (xh != nullptr) != (gamma != nullptr))
        return -2;
    DBuf dc, de, dtab, dptrs, dpad, dg;
    if (!dc.up(codes16, (size_t)R * 16 * 4) || !de.up(talker_emb, (size_t)talker_vocab * H * 4) ||
        !upload_tables(cp_tables, n_groups, cp_vocab, H, dtab, dptrs))
        return -1;
    if (pad && !dpad.up(pad, (size_t)H * 4)) return -1;
    if (gamma && !dg.up(gamma, (size_t)H * 4)) return -1;
    RowOut o;
    if (!o.init(R, H, true, true, xh != nullptr)) return -1;
    Q3_HIP(hipDeviceSynchronize(), -1);
    if (launch_feedback(nullptr, (const int*)dc.p, R, (const float*)de.p, talker_vocab, (const float* const*)dptrs.p, cp_vocab,
                        n_groups, pad ? (const float*)dpad.p : nullptr, o.ph(), o.ps(), H, o.px(), gamma ? (const float*)dg.p : nullptr))
        return -1;
    Q3_HIP(hipDeviceSynchronize(), -1);
    const int c = o.collect([&](int r) { return r < R; }, h, ssq, xh);
    return c < 0 ? -1 : c ? -3 : 0;
}

// One launch_prompt_rows: codes[T][16]; the slot's ring past[32] and counter n_past[1] in and out; tables as in
// q3t_feedback_case (n_tab of them on the device; n_groups is what the launch is told).  Rows row0 .. row0+T-1 of buffers of
// buf_rows rows (>= row0 + T; the launch is told max_rows): with_h != 0 builds them into h[buf_rows][H], ssq and -- with
// gamma -- xh, which come back for those rows; with_h == 0 passes h = null (only the ring and the counter may change).
// null_table: 1 passes talker_emb = null, 2 cp_tables = null (the launcher's refusals).  A refusal (-1) still brings the ring
// and the counter back and checks every guard.  Guards and the other return codes as q3t_final_norm_case.
static int prompt_rows_case(const int* codes, int T, int* past, int* n_past, const float* talker_emb, int talker_vocab,
                            const float* cp_tables, int n_tab, int cp_vocab, int n_groups, const float* pad, int H,
                            int row0, int max_rows, int buf_rows, int with_h, const float* gamma, float* h, float* ssq,
                            uint16_t* xh, int null_table, unsigned* seen, int seen_vocab) {
    if (!codes || T <= 0 || !past || !n_past || !talker_emb || talker_vocab <= 0 || !cp_tables || n_tab < 1 || n_tab > 15 ||
        cp_vocab <= 0 || H <= 0 || H % 32 || row0 < 0 || buf_rows < row0 + T)
        return -2;
    if (with_h ? (!h || !ssq || (xh != nullptr) != (gamma != nullptr)) : (xh || gamma)) return -2;
    // ids as the caller of launch_prompt_rows has checked them
    for (int i = 0; i < T; i++)
        for (int g = 0; g < 16; g++)
            if (codes[i * 16 + g] < 0 || codes[i * 16 + g] >= (g ? cp_vocab : talker_vocab)) return -2;
    std::vector<int> cpad((size_t)T * 16 + 16, 0);   // (one frame of slack behind the ids)
    memcpy(cpad.data(), codes, (size_t)T * 16 * 4);
    DBuf dc, dpast, dn, de, dtab, dptrs, dpad, dg, dseen;
    const size_t seen_words = seen_vocab > 0 ? ((size_t)seen_vocab + 31) / 32 : 0;
    if (seen && (seen_vocab <= 0 || !dseen.up(seen, seen_words * 4))) return seen_vocab <= 0 ? -2 : -1;
    if (!dc.up(cpad.data(), cpad.size() * 4) || !dpast.up(past, 32 * 4) || !dn.up(n_past, 4) ||
        !de.up(talker_emb, (size_t)talker_vocab * H * 4) || !upload_tables(cp_tables, n_tab, cp_vocab, H, dtab, dptrs))
        return -1;
    if (pad && !dpad.up(pad, (size_t)H * 4)) return -1;
    if (gamma && !dg.up(gamma, (size_t)H * 4)) return -1;
    RowOut o;
    if (!o.init(buf_rows, H, true, true, xh != nullptr)) return -1;
    PromptRowsArgs a;
    a.codes = (const int*)dc.p;
    a.T = T;
    a.past = (int*)dpast.p;
    a.n_past = (int*)dn.p;
    a.talker_emb = null_table == 1 ? nullptr : (const float*)de.p;
    a.talker_vocab = talker_vocab;
    a.cp_tables = null_table == 2 ? nullptr : (const float* const*)dptrs.p;
    a.cp_vocab = cp_vocab;
    a.n_groups = n_groups;
    a.pad_embed = pad ? (const float*)dpad.p : nullptr;
    if (with_h) {
        a.h = o.ph();
        a.ssq = o.ps();
        a.xh = o.px();
        a.gamma = gamma ? (const float*)dg.p : nullptr;
    }
    a.row0 = row0;
    a.max_rows = max_rows;
    a.H = H;
    a.seen = seen ? (unsigned*)dseen.p : nullptr;
    a.seen_vocab = seen ? seen_vocab : 0;
    Q3_HIP(hipDeviceSynchronize(), -1);
    const int rc = launch_prompt_rows(nullptr, a);
    Q3_HIP(hipDeviceSynchronize(), -1);
    if (seen) Q3_HIP(hipMemcpy(seen, dseen.p, seen_words * 4, hipMemcpyDeviceToHost), -1);
    Q3_HIP(hipMemcpy(past, dpast.p, 32 * 4, hipMemcpyDeviceToHost), -1);
    Q3_HIP(hipMemcpy(n_past, dn.p, 4, hipMemcpyDeviceToHost), -1);
    const bool built = with_h && rc == 0;
    const int c = o.collect([&](int r) { return built && r >= row0 && r < row0 + T; }, h, ssq, xh);
    return c < 0 ? -1 : c ? -3 : rc;
}
extern "C" int q3t_prompt_rows_case(const int* codes, int T, int* past, int* n_past, const float* talker_emb, int talker_vocab,
                                    const float* cp_tables, int n_tab, int cp_vocab, int n_groups, const float* pad, int H,
                                    int row0, int max_rows, int buf_rows, int with_h, const float* gamma, float* h, float* ssq,
                                    uint16_t* xh, int null_table) {
    return prompt_rows_case(codes, T, past, n_past, talker_emb, talker_vocab, cp_tables, n_tab, cp_vocab, n_groups, pad, H, row0,
                            max_rows, buf_rows, with_h, gamma, h, ssq, xh, null_table, nullptr, 0);
}
// q3t_prompt_rows_case with the slot's seen-set (PromptRowsArgs::seen / seen_vocab): seen[(seen_vocab + 31) / 32] in and out.
extern "C" int q3t_prompt_rows_seen_case(const int* codes, int T, int* past, int* n_past, const float* talker_emb,
                                         int talker_vocab, const float* cp_tables, int n_tab, int cp_vocab, int n_groups,
                                         const float* pad, int H, int row0, int max_rows, int buf_rows, int with_h,
                                         const float* gamma, float* h, float* ssq, uint16_t* xh, int null_table, unsigned* seen,
                                         int seen_vocab) {
    return prompt_rows_case(codes, T, past, n_past, talker_emb, talker_vocab, cp_tables, n_tab, cp_vocab, n_groups, pad, H, row0,
                            max_rows, buf_rows, with_h, gamma, h, ssq, xh, null_table, seen, seen_vocab);
}

// One launch_prefix_move on host arrays, everything in and out whole: caches kc / vc [n_layers][n_slots][n_kv][n_ctx][128]
// (fp16 bits), pool[n_entries][n_layers][2][n_kv][max_rows][128], states[n_entries][H + H/16], h[h_rows][H] (row-major here,
// fragment order on the device) and ssq[h_rows][H/16].  launch = {n_layers, n_kv, n_ctx, max_rows, H, slot, n_rows, h_row,
// restore, null} is what the launch is told (null: bit i nulls kc, vc, entry, state, h, ssq): a set the launcher accepts must
// lie inside the buffers (-2 otherwise); one it refuses (-1) still brings everything back.  -3: the guard rows behind kc, vc,
// the pool or h changed.
extern "C" int q3t_prefix_move_case(uint16_t* kc, uint16_t* vc, int n_layers, int n_slots, int n_kv, int n_ctx, uint16_t* pool,
                                    int n_entries, int max_rows, float* states, float* h, float* ssq, int h_rows, int H, int entry,
                                    const int* launch) {
    if (!kc || !vc || !pool || !states || !h || !ssq || !launch || n_layers <= 0 || n_slots <= 0 || n_kv <= 0 || n_ctx <= 0 ||
        n_entries <= 0 || max_rows <= 0 || h_rows <= 0 || H <= 0 || H % 32 || entry < 0 || entry >= n_entries)
        return -2;
    const int l_layers = launch[0], l_kv = launch[1], l_ctx = launch[2], l_max = launch[3], l_H = launch[4], slot = launch[5],
              n_rows = launch[6], h_row = launch[7], restore = launch[8], nul = launch[9];
    const bool refused = nul || l_layers <= 0 || l_kv <= 0 || slot < 0 || n_rows <= 0 || n_rows > l_ctx || n_rows > l_max || h_row < 0 ||
                         l_H <= 0 || l_H % 32;
    if (!refused && (l_layers > n_layers || l_kv != n_kv || l_ctx != n_ctx || l_max != max_rows || l_H != H || slot >= n_slots ||
                     h_row >= h_rows))
        return -2;
    constexpr size_t TAIL = 16 * 128;   // guard rows behind every fp16 buffer
    const size_t layer = (size_t)n_slots * n_kv * n_ctx * 128, nc = (size_t)n_layers * layer;
    const size_t ent = (size_t)n_layers * 2 * n_kv * max_rows * 128, np = (size_t)n_entries * ent;
    const int parts = H / 16, Rp = (h_rows + 15) / 16 * 16;
    std::vector<uint16_t> hk(nc + TAIL, ROW_GUARD16), hv(nc + TAIL, ROW_GUARD16), hpool(np + TAIL, ROW_GUARD16);
    memcpy(hk.data(), kc, nc * 2);
    memcpy(hv.data(), vc, nc * 2);
    memcpy(hpool.data(), pool, np * 2);
    std::vector<uint32_t> hh((size_t)Rp * H, ROW_GUARD32), hs((size_t)Rp * parts, ROW_GUARD32);
    for (int r = 0; r < h_rows; r++) {
        for (int k = 0; k < H; k++) memcpy(&hh[frag_idx(r, k, H)], &h[(size_t)r * H + k], 4);
        memcpy(&hs[(size_t)r * parts], &ssq[(size_t)r * parts], (size_t)parts * 4);
    }
    const size_t nst = (size_t)n_entries * (H + parts);
    DBuf dk, dv, dp, dst, dh, ds;
    if (!dk.up(hk.data(), hk.size() * 2) || !dv.up(hv.data(), hv.size() * 2) || !dp.up(hpool.data(), hpool.size() * 2) ||
        !dst.up(states, nst * 4) || !dh.up(hh.data(), hh.size() * 4) || !ds.up(hs.data(), hs.size() * 4))
        return -1;
    PrefixMoveArgs a;
    a.kc = (nul & 1) ? nullptr : (half_t*)dk.p;
    a.vc = (nul & 2) ? nullptr : (half_t*)dv.p;
    a.layer_stride = layer;
    a.n_layers = l_layers;
    a.n_kv = l_kv;
    a.n_ctx = l_ctx;
    a.slot = slot;
    a.n_rows = n_rows;
    a.entry = (nul & 4) ? nullptr : (half_t*)dp.p + (size_t)entry * ent;
    a.max_rows = l_max;
    a.state = (nul & 8) ? nullptr : (float*)dst.p + (size_t)entry * (H + parts);
    a.h = (nul & 16) ? nullptr : (float*)dh.p;
    a.ssq = (nul & 32) ? nullptr : (float*)ds.p;
    a.h_row = h_row;
    a.H = l_H;
    a.restore = restore;
    Q3_HIP(hipDeviceSynchronize(), -1);
    const int rc = launch_prefix_move(nullptr, a);
    Q3_HIP(hipDeviceSynchronize(), -1);
    Q3_HIP(hipMemcpy(hk.data(), dk.p, hk.size() * 2, hipMemcpyDeviceToHost), -1);
    Q3_HIP(hipMemcpy(hv.data(), dv.p, hv.size() * 2, hipMemcpyDeviceToHost), -1);
    Q3_HIP(hipMemcpy(hpool.data(), dp.p, hpool.size() * 2, hipMemcpyDeviceToHost), -1);
    Q3_HIP(hipMemcpy(states, dst.p, nst * 4, hipMemcpyDeviceToHost), -1);
    Q3_HIP(hipMemcpy(hh.data(), dh.p, hh.size() * 4, hipMemcpyDeviceToHost), -1);
    Q3_HIP(hipMemcpy(hs.data(), ds.p, hs.size() * 4, hipMemcpyDeviceToHost), -1);
    memcpy(kc, hk.data(), nc * 2);
    memcpy(vc, hv.data(), nc * 2);
    memcpy(pool, hpool.data(), np * 2);
    int outside = 0;
    for (size_t i = 0; i < TAIL; i++) outside += (hk[nc + i] != ROW_GUARD16) + (hv[nc + i] != ROW_GUARD16) + (hpool[np + i] != ROW_GUARD16);
    for (int r = 0; r < Rp; r++) {
        for (int k = 0; k < H; k++) {
            const uint32_t v = hh[frag_idx(r, k, H)];
            if (r < h_rows) memcpy(&h[(size_t)r * H + k], &v, 4);
            else outside += v != ROW_GUARD32;
        }
        for (int p = 0; p < parts; p++) {
            const uint32_t v = hs[(size_t)r * parts + p];
            if (r < h_rows) memcpy(&ssq[(size_t)r * parts + p], &v, 4);
            else outside += v != ROW_GUARD32;
        }
    }
    return outside ? -3 : rc;
}

// ---- the speaker encoder's stages (q3_spk.hip): the log-mel [B][n_mels][L] and the activation after a stage [B][C][L]
// (L = the longest clip's frames; the pooled stages asp and fc: [B][C], L = 1).  Stage 0 block0, 1.. the SE-Res2Net blocks,
// then mfa, asp, fc.  out is sized by the caller for the call's lengths (spk_frames); 0 / <0
extern "C" int q3t_spk_mel(void* h, const float* pcm, const int32_t* n_samples, int B, float* out, int* C, int* L) {
    return spk_debug_mel((Spk*)h, pcm, n_samples, B, out, C, L);
}
extern "C" int q3t_spk_stage(void* h, const float* pcm, const int32_t* n_samples, int B, int stage, float* out, int* C, int* L) {
    return spk_debug_stage((Spk*)h, pcm, n_samples, B, stage, out, C, L);
}

// ---- launch_dequant (q3_dequant.hip) on rows [row0, row0 + rows) of a tensor of rows_total x K elements of a ggml block
// type (DType Q4_0 .. Q6_K), whose raw blocks are `blocks` (nbytes = rows_total * K / block * block bytes).  out16 (fp16
// bits) or out32, whichever is not null: [rows][K].  *flag: what the launch left in its device flag (zeroed before).
// 0, -1 HIP, -2 arguments, -3 something was written behind the rows asked for.
extern "C" int q3t_dequant_case(int type, const uint8_t* blocks, long long nbytes, int rows_total, int K, int row0, int rows,
                                uint16_t* out16, float* out32, int* flag) {
    const BlockGeom g = block_geom((uint32_t)type);
    if (!is_block_dtype((uint32_t)type) || !blocks || !flag || (out16 != nullptr) == (out32 != nullptr) || K <= 0 || K % (int)g.elems ||
        rows_total < 1 || rows < 1 || row0 < 0 || row0 + rows > rows_total)
        return -2;
    const size_t row_bytes = (size_t)K / g.elems * g.bytes;
    if ((long long)(row_bytes * rows_total) != nbytes) return -2;
    constexpr uint32_t GUARD = 0x7fc5a5a5u;
    const size_t n = (size_t)rows * K, esz = out16 ? 2 : 4, tail = 64;
    std::vector<uint32_t> ho((n * esz + tail) / 4 + 1, GUARD);
    DBuf db, dout, df;
    int zero = 0;
    if (!db.up(blocks, (size_t)nbytes) || !dout.up(ho.data(), ho.size() * 4) || !df.up(&zero, 4)) return -1;
    Q3_HIP(hipDeviceSynchronize(), -1);
    if (launch_dequant(nullptr, (uint32_t)type, (const uint8_t*)db.p + (size_t)row0 * row_bytes, (size_t)rows, (size_t)K,
                       out16 ? (half_t*)dout.p : nullptr, out32 ? (float*)dout.p : nullptr, (int*)df.p))
        return -1;
    Q3_HIP(hipDeviceSynchronize(), -1);
    Q3_HIP(hipMemcpy(ho.data(), dout.p, ho.size() * 4, hipMemcpyDeviceToHost), -1);
    Q3_HIP(hipMemcpy(flag, df.p, 4, hipMemcpyDeviceToHost), -1);
    memcpy(out16 ? (void*)out16 : (void*)out32, ho.data(), n * esz);
    for (size_t i = n * esz / 4; i < ho.size(); i++)   // n * esz is a multiple of 16
        if (ho[i] != GUARD) return -3;
    return 0;
}

// ---- the speaker encoder's own kernels (csrc/q3_spk.hip), one launch each (tests/test_gpu_spk_ops.py) ----------------
// Conventions of q3t_enc_conv_in_case.  Activations are dense on the host and rows of the production pitch on the device
// (ld = spk_pitch of the call's longest clip).  A kernel that stops at the clip's own length (unfold, rowmean, rowstat,
// attnpool) takes [B][C][Lmax] and finds NaN in the pad columns [Lmax, ld); a kernel that runs over every column of the
// pitch (place, se_apply, att_act) takes and returns [B][C][ld], ld = spk_pitch(L).  Every output is the guard pattern
// before the launch: 32 words behind each buffer and the channels of a sliced destination outside the slice must keep it
// (-3).  -2: arguments the walk never passes, before anything launches; -1: a HIP error.
namespace {
constexpr uint32_t OP_GUARD = 0x7fc5a5a5u;
constexpr long long OP_MAX_WORDS = 1LL << 27;

std::vector<float> op_padded(const float* src, size_t rows, int n, int ld) {
    std::vector<float> h(rows * ld, std::nanf(""));
    for (size_t r = 0; r < rows; r++) memcpy(h.data() + r * ld, src + r * n, (size_t)n * 4);
    return h;
}
struct OpOut {
    std::vector<uint32_t> h;
    DBuf d;
    size_t words = 0;
    bool init(size_t w) {
        words = w;
        h.assign(w + 32, OP_GUARD);
        return d.up(h.data(), h.size() * 4);
    }
    float* p() { return (float*)d.p; }
    bool down() { return hipMemcpy(h.data(), d.p, h.size() * 4, hipMemcpyDeviceToHost) == hipSuccess; }
    int tail() const {
        int n = 0;
        for (size_t i = words; i < h.size(); i++) n += h[i] != OP_GUARD;
        return n;
    }
    // channels [c0, c0 + C) of [B][Ct][ld] go to dst [B][C][ld]; -> the words outside them that lost their guard
    int slice(float* dst, int B, int Ct, int c0, int C, int ld) const {
        int n = tail();
        for (int b = 0; b < B; b++)
            for (int c = 0; c < Ct; c++) {
                const uint32_t* row = h.data() + ((size_t)b * Ct + c) * ld;
                if (c >= c0 && c < c0 + C) memcpy(dst + ((size_t)b * C + c - c0) * ld, row, (size_t)ld * 4);
                else
                    for (int l = 0; l < ld; l++) n += row[l] != OP_GUARD;
            }
        return n;
    }
};
// the clips' frame counts: all >= lo -> the longest, or -1
int op_longest(const int* n_f, int B, int lo) {
    if (!n_f || B < 1 || B > 65535) return -1;
    int L = 0;
    for (int b = 0; b < B; b++) {
        if (n_f[b] < lo || n_f[b] > (1 << 20)) return -1;
        L = std::max(L, n_f[b]);
    }
    return L;
}
}  // namespace

// x [B][Cx][Lmax] (+ x2 [B][Cx2][Lmax] or null) -> y [B][C * K][ld], every column of the pitch
extern "C" int q3t_spk_unfold_case(const float* x, int Cx, int c0, const float* x2, int Cx2, int c02, const int* n_f, int B, int C, int K,
                                   int dil, float* y) {
    if (!x || !y || C < 1 || K < 1 || K > 15 || !(K & 1) || dil < 1 || dil > 64 || c0 < 0 || Cx < 1 || c0 + C > Cx) return -2;
    if (x2 && (c02 < 0 || Cx2 < 1 || c02 + C > Cx2)) return -2;
    const int L = op_longest(n_f, B, dil * (K - 1) / 2 + 1);   // (the reflection stays inside the clip: spk_load's min_frames)
    if (L < 0 || (long long)C * K > 65535) return -2;
    const int ld = (int)spk_pitch(L);
    if ((long long)B * std::max(std::max(Cx, Cx2), C * K) * ld > OP_MAX_WORDS) return -2;
    const std::vector<float> hx = op_padded(x, (size_t)B * Cx, L, ld);
    DBuf dx, dx2, dn;
    OpOut o;
    if (!dx.up(hx.data(), hx.size() * 4) || !dn.up(n_f, (size_t)B * 4) || !o.init((size_t)B * C * K * ld)) return -1;
    if (x2) {
        const std::vector<float> hx2 = op_padded(x2, (size_t)B * Cx2, L, ld);
        if (!dx2.up(hx2.data(), hx2.size() * 4)) return -1;
    }
    Q3_HIP(hipDeviceSynchronize(), -1);
    if (spk_launch_unfold(nullptr, (const float*)dx.p, Cx, c0, x2 ? (const float*)dx2.p : nullptr, Cx2, c02, (const int*)dn.p, o.p(), C, K, dil,
                          ld, B))
        return -1;
    Q3_HIP(hipDeviceSynchronize(), -1);
    if (!o.down()) return -1;
    memcpy(y, o.h.data(), o.words * 4);
    return o.tail() ? -3 : 0;
}

// channels [c0x, c0x + C) of x [B][Cx][ld] -> channels [c0y, c0y + C) of a [B][Cy][ld] destination; y [B][C][ld] is that slice
extern "C" int q3t_spk_place_case(const float* x, int Cx, int c0x, int Cy, int c0y, int C, int L, int relu, int B, float* y) {
    if (!x || !y || B < 1 || B > 65535 || C < 1 || C > 65535 || L < 1 || L > (1 << 20) || c0x < 0 || c0x + C > Cx || c0y < 0 || c0y + C > Cy ||
        (relu != 0 && relu != 1))
        return -2;
    const int ld = (int)spk_pitch(L);
    if ((long long)B * std::max(Cx, Cy) * ld > OP_MAX_WORDS) return -2;
    DBuf dx;
    OpOut o;
    if (!dx.up(x, (size_t)B * Cx * ld * 4) || !o.init((size_t)B * Cy * ld)) return -1;
    Q3_HIP(hipDeviceSynchronize(), -1);
    if (spk_launch_place(nullptr, (const float*)dx.p, Cx, c0x, o.p(), Cy, c0y, C, ld, relu, B)) return -1;
    Q3_HIP(hipDeviceSynchronize(), -1);
    if (!o.down()) return -1;
    return o.slice(y, B, Cy, c0y, C, ld) ? -3 : 0;
}

// the three one-wave-per-row reductions.  which 0: spk_rowmean -> out [B][C]; 1: spk_rowstat -> out [B][2 C];
// 2: spk_attnpool (z = the logits) -> out [B][2 C].  x (and z) [B][C][Lmax]
static int spk_reduce_case(int which, const float* z, const float* x, int C, const int* n_f, int B, float* out) {
    if (!x || !out || (which == 2 && !z) || C < 1 || C > 4 * 65535) return -2;
    const int L = op_longest(n_f, B, 1);
    if (L < 0) return -2;
    const int ld = (int)spk_pitch(L);
    if ((long long)B * C * ld > OP_MAX_WORDS) return -2;
    const std::vector<float> hx = op_padded(x, (size_t)B * C, L, ld);
    DBuf dx, dz, dn;
    OpOut o;
    if (!dx.up(hx.data(), hx.size() * 4) || !dn.up(n_f, (size_t)B * 4) || !o.init((size_t)B * C * (which ? 2 : 1))) return -1;
    if (which == 2) {
        const std::vector<float> hz = op_padded(z, (size_t)B * C, L, ld);
        if (!dz.up(hz.data(), hz.size() * 4)) return -1;
    }
    Q3_HIP(hipDeviceSynchronize(), -1);
    const float* X = (const float*)dx.p;
    const int* N = (const int*)dn.p;
    const int rc = which == 0 ? spk_launch_rowmean(nullptr, X, C, ld, N, o.p(), B)
                   : which == 1 ? spk_launch_rowstat(nullptr, X, C, ld, N, o.p(), B)
                                : spk_launch_attnpool(nullptr, (const float*)dz.p, X, C, ld, N, o.p(), B);
    if (rc) return -1;
    Q3_HIP(hipDeviceSynchronize(), -1);
    if (!o.down()) return -1;
    memcpy(out, o.h.data(), o.words * 4);
    return o.tail() ? -3 : 0;
}
extern "C" int q3t_spk_rowmean_case(const float* x, int C, const int* n_f, int B, float* out) { return spk_reduce_case(0, nullptr, x, C, n_f, B, out); }
extern "C" int q3t_spk_rowstat_case(const float* x, int C, const int* n_f, int B, float* stat) { return spk_reduce_case(1, nullptr, x, C, n_f, B, stat); }
extern "C" int q3t_spk_attnpool_case(const float* z, const float* x, int C, const int* n_f, int B, float* pooled) {
    return spk_reduce_case(2, z, x, C, n_f, B, pooled);
}

// w [O][I], bias [O] or null, in [B][I] -> out [B][O]
extern "C" int q3t_spk_matvec_case(const float* w, const float* bias, const float* in, int I, int O, int act, int B, float* out) {
    if (!w || !in || !out || I < 1 || O < 1 || O > 4 * 65535 || B < 1 || B > 65535 || act < 0 || act > 2 || (long long)I * O > OP_MAX_WORDS ||
        (long long)B * std::max(I, O) > OP_MAX_WORDS)
        return -2;
    DBuf dw, db, di;
    OpOut o;
    if (!dw.up(w, (size_t)I * O * 4) || !di.up(in, (size_t)B * I * 4) || !o.init((size_t)B * O)) return -1;
    if (bias && !db.up(bias, (size_t)O * 4)) return -1;
    Q3_HIP(hipDeviceSynchronize(), -1);
    if (spk_launch_matvec(nullptr, (const float*)dw.p, bias ? (const float*)db.p : nullptr, (const float*)di.p, o.p(), I, O, act, B)) return -1;
    Q3_HIP(hipDeviceSynchronize(), -1);
    if (!o.down()) return -1;
    memcpy(out, o.h.data(), o.words * 4);
    return o.tail() ? -3 : 0;
}

// h, res [B][C][ld], gate [B][C] -> y1 [B][C][ld] and channels [c02, c02 + C) of a [B][Cy2][ld] aggregate; y2 [B][C][ld] is that slice
extern "C" int q3t_spk_se_apply_case(const float* h, const float* gate, const float* res, int C, int L, int Cy2, int c02, int B, float* y1,
                                     float* y2) {
    if (!h || !gate || !res || !y1 || !y2 || B < 1 || B > 65535 || C < 1 || C > 65535 || L < 1 || L > (1 << 20) || c02 < 0 || c02 + C > Cy2)
        return -2;
    const int ld = (int)spk_pitch(L);
    if ((long long)B * Cy2 * ld > OP_MAX_WORDS) return -2;
    const size_t n = (size_t)B * C * ld;
    DBuf dh, dg, dr;
    OpOut o1, o2;
    if (!dh.up(h, n * 4) || !dg.up(gate, (size_t)B * C * 4) || !dr.up(res, n * 4) || !o1.init(n) || !o2.init((size_t)B * Cy2 * ld)) return -1;
    Q3_HIP(hipDeviceSynchronize(), -1);
    if (spk_launch_se_apply(nullptr, (const float*)dh.p, (const float*)dg.p, (const float*)dr.p, o1.p(), o2.p(), Cy2, c02, C, ld, B)) return -1;
    Q3_HIP(hipDeviceSynchronize(), -1);
    if (!o1.down() || !o2.down()) return -1;
    memcpy(y1, o1.h.data(), n * 4);
    return (o1.tail() + o2.slice(y2, B, Cy2, c02, C, ld)) ? -3 : 0;
}

// x [B][C][ld], bias [B][C] -> y [B][C][ld]
extern "C" int q3t_spk_att_act_case(const float* x, const float* bias, int C, int L, int B, float* y) {
    if (!x || !bias || !y || B < 1 || B > 65535 || C < 1 || C > 65535 || L < 1 || L > (1 << 20)) return -2;
    const int ld = (int)spk_pitch(L);
    if ((long long)B * C * ld > OP_MAX_WORDS) return -2;
    const size_t n = (size_t)B * C * ld;
    DBuf dx, db;
    OpOut o;
    if (!dx.up(x, n * 4) || !db.up(bias, (size_t)B * C * 4) || !o.init(n)) return -1;
    Q3_HIP(hipDeviceSynchronize(), -1);
    if (spk_launch_att_act(nullptr, (const float*)dx.p, (const float*)db.p, o.p(), C, ld, B)) return -1;
    Q3_HIP(hipDeviceSynchronize(), -1);
    if (!o.down()) return -1;
    memcpy(y, o.h.data(), n * 4);
    return o.tail() ? -3 : 0;
}

// ---- the encoder's unfold and emit kernels (csrc/q3_enc.hip, csrc/q3_enc_stream.hip), one launch each (tests/test_gpu_enc_unfold.py) ----
// x [B][Cin][Lmax] (Lmax = the longest of lens; NaN in the pad columns of the pitch) -> y [B][Cin * k][Lout], Lout = ceil(Lmax / s);
// the columns of y's pitch from Lout on keep their guard (-3)
extern "C" int q3t_enc_unfold_case(const float* x, int B, int Cin, const int* lens, int k, int s, int replicate, int elu, float* y) {
    if (!x || !y || Cin < 1 || s < 1 || k < s || k > 64 || (long long)Cin * k > 65535 || (replicate & ~1) || (elu & ~1)) return -2;
    const int L = op_longest(lens, B, 1);
    if (L < 0) return -2;
    const int Lout = (L + s - 1) / s, ldx = (int)enc_pitch(L), ldy = (int)enc_pitch(Lout);
    const size_t rows = (size_t)B * Cin * k;
    if ((long long)rows * ldy > OP_MAX_WORDS || (long long)B * Cin * ldx > OP_MAX_WORDS) return -2;
    const std::vector<float> hx = op_padded(x, (size_t)B * Cin, L, ldx);
    DBuf dx, dn;
    OpOut o;
    if (!dx.up(hx.data(), hx.size() * 4) || !dn.up(lens, (size_t)B * 4) || !o.init(rows * ldy)) return -1;
    Q3_HIP(hipDeviceSynchronize(), -1);
    if (enc_launch_unfold(nullptr, (const float*)dx.p, ldx, Cin, (const int*)dn.p, o.p(), Lout, k, s, replicate, elu, B)) return -1;
    Q3_HIP(hipDeviceSynchronize(), -1);
    if (!o.down()) return -1;
    int outside = o.tail();
    for (size_t r = 0; r < rows; r++) {
        memcpy(y + r * Lout, o.h.data() + r * ldy, (size_t)Lout * 4);
        for (int l = Lout; l < ldy; l++) outside += o.h[r * ldy + l] != OP_GUARD;
    }
    return outside ? -3 : 0;
}

// One push of enc_stream_unfold_kernel.  x [B][Cin][skip + n_in] (the skipped columns are the caller's; NaN in the pad),
// entry b continues stream streams[b] (distinct, < max_streams) that had taken before[b] columns; hist [max_streams][Cin][k - 1]
// goes in and the named streams' rows come back as the launch left them (the other streams' rows hold the guard on the device
// and must keep it).  -> y [B][Cin * k][n_out].  -2 also: a before[b] that does not give n_out, and n_in = n_out = 0 (the walk
// launches nothing then).
extern "C" int q3t_enc_stream_unfold_case(const float* x, int B, int Cin, int skip, int n_in, int n_out, int k, int s, int replicate, int elu,
                                          int finish, float* hist, int max_streams, const int* streams, const int* before, float* y) {
    if (!x || !y || !hist || !streams || !before || B < 1 || B > 65535 || Cin < 1 || Cin > 65535 || s < 1 || k < s || k - 1 > 32 || skip < 0 ||
        n_in < 0 || n_out < 0 || (n_in == 0 && n_out == 0) || max_streams < B || (replicate & ~1) || (elu & ~1) || (finish & ~1))
        return -2;
    if ((long long)skip + n_in > (1 << 20) || (long long)max_streams * Cin * (k - 1) > OP_MAX_WORDS) return -2;
    std::vector<char> seen((size_t)max_streams, 0);
    for (int b = 0; b < B; b++) {
        if (streams[b] < 0 || streams[b] >= max_streams || seen[(size_t)streams[b]]++ || before[b] < 0 || before[b] > 0x7fffffff - n_in) return -2;
        const long long after = (long long)before[b] + n_in;
        if ((finish ? (after + s - 1) / s : after / s) - before[b] / s != n_out) return -2;
    }
    const int cols = skip + n_in, ldx = (int)enc_pitch(cols), ldy = (int)enc_pitch(n_out), H = k - 1;
    const size_t rows = (size_t)B * Cin * k, sf = (size_t)Cin * H, nh = (size_t)max_streams * sf;
    if ((long long)rows * ldy > OP_MAX_WORDS || (long long)B * Cin * ldx > OP_MAX_WORDS) return -2;
    const std::vector<float> hx = op_padded(x, (size_t)B * Cin, cols, ldx);
    OpOut o, oh;
    DBuf dx, ds, db;
    if (!dx.up(hx.data(), hx.size() * 4) || !ds.up(streams, (size_t)B * 4) || !db.up(before, (size_t)B * 4) || !o.init(rows * ldy)) return -1;
    oh.words = nh;
    oh.h.assign(nh + 32, OP_GUARD);
    for (int b = 0; b < B; b++) memcpy(oh.h.data() + (size_t)streams[b] * sf, hist + (size_t)streams[b] * sf, sf * 4);
    if (!oh.d.up(oh.h.data(), oh.h.size() * 4)) return -1;
    Q3_HIP(hipDeviceSynchronize(), -1);
    if (enc_stream_launch_unfold(nullptr, (const float*)dx.p, ldx, skip, Cin, n_in, o.p(), n_out, k, s, replicate, elu, finish, oh.p(),
                                 (long long)sf, (const int*)ds.p, (const int*)db.p, B))
        return -1;
    Q3_HIP(hipDeviceSynchronize(), -1);
    if (!o.down() || !oh.down()) return -1;
    int outside = o.tail() + oh.tail();
    for (size_t r = 0; r < rows; r++) {
        memcpy(y + r * n_out, o.h.data() + r * ldy, (size_t)n_out * 4);
        for (int l = n_out; l < ldy; l++) outside += o.h[r * ldy + l] != OP_GUARD;
    }
    for (int st = 0; st < max_streams; st++) {
        if (seen[(size_t)st]) memcpy(hist + (size_t)st * sf, oh.h.data() + (size_t)st * sf, sf * 4);
        else
            for (size_t i = 0; i < sf; i++) outside += oh.h[(size_t)st * sf + i] != OP_GUARD;
    }
    return outside ? -3 : 0;
}

// columns [skip, skip + n) of y [B][C][skip + n] -> rows off[b] .. off[b] + n - 1 of out [rows][C] (disjoint, inside `rows`); out comes
// back whole: the rows no entry owns hold the guard pattern, and must (-3)
extern "C" int q3t_enc_stream_emit_case(const float* y, int B, int C, int skip, int n, const int* off, int rows, float* out) {
    if (!y || !off || !out || B < 1 || B > 65535 || C < 1 || skip < 0 || n < 1 || n > 65535 || rows < 1 || (long long)rows * C > OP_MAX_WORDS ||
        (long long)B * C * enc_pitch((long)skip + n) > OP_MAX_WORDS)
        return -2;
    std::vector<char> owned((size_t)rows, 0);
    for (int b = 0; b < B; b++) {
        if (off[b] < 0 || (long long)off[b] + n > rows) return -2;
        for (int j = 0; j < n; j++)
            if (owned[(size_t)off[b] + j]++) return -2;
    }
    const int cols = skip + n, ld = (int)enc_pitch(cols);
    const std::vector<float> hy = op_padded(y, (size_t)B * C, cols, ld);
    DBuf dy, dn;
    OpOut o;
    if (!dy.up(hy.data(), hy.size() * 4) || !dn.up(off, (size_t)B * 4) || !o.init((size_t)rows * C)) return -1;
    Q3_HIP(hipDeviceSynchronize(), -1);
    if (enc_stream_launch_emit(nullptr, (const float*)dy.p, C, ld, skip, n, (const int*)dn.p, o.p(), B)) return -1;
    Q3_HIP(hipDeviceSynchronize(), -1);
    if (!o.down()) return -1;
    memcpy(out, o.h.data(), o.words * 4);
    int outside = o.tail();
    for (int r = 0; r < rows; r++)
        if (!owned[(size_t)r])
            for (int c = 0; c < C; c++) outside += o.h[(size_t)r * C + c] != OP_GUARD;
    return outside ? -3 : 0;
}
