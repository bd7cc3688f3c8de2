// q3_spk.hip -- speaker encoder (24 kHz audio -> one ECAPA-TDNN x-vector per clip) for gfx950, include/qwen3tts_spk.h.
//
// Pinned to transformers' ECAPA_TimeDelayNet (models/qwen2_5_omni) in float64 and to float64 torch.stft + the slaney filter
// bank by tests/golden/spk_golden.npz.  Activations are [B][C][ld] f32, one row per clip and channel at a
// pitch ld = the call's longest clip's frames rounded up to 32 floats; clip b's own frame count sits on the device (d_n).
//
// The log-mel front-end runs in float64 and rounds once to float32 (the PCM resampler's reason, q3_enc_pcm.hip: every host
// gets the same numbers): spk_mel_kernel, one workgroup per (clip, tile of 4 frames), the windowed frames in LDS, a direct
// DFT from double cos / sin tables made on the host at load, the filter bank read as a tensor.  About 2 GFLOP for 10 s of
// audio: float64 costs nothing that matters, so it is not optimised.
//
// The network runs in fp32.  Every conv goes through the exact-f32 MFMA launcher (voc_launch_conv) as a ONE-tap conv: the
// launcher builds 1, 2, 3 and 7 taps and none of them reflects, so a k-tap "same" reflect conv reads the cin * k rows that
// spk_unfold_kernel writes (row ci * k + j, column l = x[ci][reflect(l + j * dil - p)], reflected at the clip's OWN ends,
// zero past its own length) -- the encoder's way with its strided convs (enc_unfold_kernel).  A one-tap column depends on
// its own column only and the launcher's variant rule is pinned (Lrule, as enc_conv_args pins it), so the order of every sum
// depends on nothing in the call: clip b gives the same bits alone and in any batch.  Own kernels:
//   spk_unfold_kernel     reflect padding + unfold, with the Res2Net add (chunk_i + out_{i-1}) folded in
//   spk_place_kernel      ReLU epilogue of a conv, written into a channel slice (the Res2Net concat)
//   spk_rowmean_kernel, spk_matvec_kernel, spk_se_apply_kernel   squeeze-excitation: per-clip mean over the clip's own columns,
//                         two matvecs (ReLU, sigmoid), scale + residual (written to the next block and to the aggregate)
//   spk_rowstat_kernel    global mean and std, two passes: sum m (x - mean)^2, clamped at 1e-12 before the root
//   spk_att_act_kernel    + per-clip bias (the mean / std columns of asp.tdnn folded into a matvec), ReLU then tanh
//   spk_attnpool_kernel   softmax over the clip's own columns per channel, weighted mean and std
// Reductions are one wave per (clip, channel) row on the cross-lane helpers (q3_xlane.h): lane-strided partial sums, one
// butterfly -- a fixed tree per row, whatever the batch.
#include "../../include/qwen3tts_spk.h"
#include "q3_spk.h"
#include "q3_xlane.h"

#include <algorithm>
#include <cmath>
#include <string>

namespace q3 {

// ---------------------------------------------------------------------------
// Log-mel, float64.  Workgroup = FT frames of one clip; thread t owns the bins t, t + 256, t + 512 (n_fft <= 1024: spk_load).
// LDS: the windowed frames [FT][N] (then the magnitudes [FT][N / 2 + 1] over them), cos and sin of 2 pi j / N.
// Every sum runs in index order (j, then k): a frame's bits depend on the frame alone.
// ---------------------------------------------------------------------------
constexpr int SPK_FT = 4;
__global__ void __launch_bounds__(256) spk_mel_kernel(const float* __restrict__ pcm, int ldp, const int* __restrict__ n_s,
                                                      const int* __restrict__ n_f, const double* __restrict__ win,
                                                      const double* __restrict__ ctab, const double* __restrict__ stab,
                                                      const double* __restrict__ fb, float* __restrict__ mel, int ld, int N, int hop,
                                                      int pad, int n_mels, double mel_floor, double mag_eps) {
    extern __shared__ __attribute__((aligned(16))) double smd[];
    double* xw = smd;                 // [FT][N]
    double* ct = smd + SPK_FT * N;    // [N]
    double* st = ct + N;              // [N]
    const int tid = threadIdx.x, b = blockIdx.y, f0 = blockIdx.x * SPK_FT;
    const int F = n_f[b], n = n_s[b];
    if (f0 >= F) return;              // (uniform: the whole workgroup leaves)
    const float* xb = pcm + (size_t)b * ldp;
    for (int idx = tid; idx < SPK_FT * N; idx += 256) {
        const int f = idx / N, j = idx - f * N, fr = f0 + f;
        double v = 0.0;
        if (fr < F) {
            const int sidx = spk_reflect(fr * hop + j - pad, n);   // (pad < n and the last frame ends inside the padded clip)
            v = (double)xb[sidx] * win[j];
        }
        xw[idx] = v;
    }
    for (int j = tid; j < N; j += 256) {
        ct[j] = ctab[j];
        st[j] = stab[j];
    }
    __syncthreads();
    const int NB = N / 2 + 1;
    double mg[3][SPK_FT];
#pragma unroll
    for (int it = 0; it < 3; it++) {
        const int k = tid + it * 256;
        double re[SPK_FT], im[SPK_FT];
#pragma unroll
        for (int f = 0; f < SPK_FT; f++) re[f] = im[f] = 0.0;
        if (k < NB) {
            int idx = 0;   // (j * k) mod N
            for (int j = 0; j < N; j++) {
                const double c = ct[idx], s = st[idx];
#pragma unroll
                for (int f = 0; f < SPK_FT; f++) {
                    const double x = xw[f * N + j];
                    re[f] = fma(x, c, re[f]);
                    im[f] = fma(x, s, im[f]);
                }
                idx += k;
                if (idx >= N) idx -= N;
            }
        }
#pragma unroll
        for (int f = 0; f < SPK_FT; f++) mg[it][f] = sqrt(re[f] * re[f] + im[f] * im[f] + mag_eps);
    }
    __syncthreads();   // every thread is done with the frames: the magnitudes go over them
#pragma unroll
    for (int it = 0; it < 3; it++) {
        const int k = tid + it * 256;
        if (k < NB) {
#pragma unroll
            for (int f = 0; f < SPK_FT; f++) xw[f * NB + k] = mg[it][f];
        }
    }
    __syncthreads();
    for (int idx = tid; idx < SPK_FT * n_mels; idx += 256) {
        const int f = idx / n_mels, m = idx - f * n_mels;
        if (f0 + f >= F) continue;
        double acc = 0.0;
        for (int k = 0; k < NB; k++) acc = fma(fb[(size_t)k * n_mels + m], xw[f * NB + k], acc);
        mel[((size_t)b * n_mels + m) * ld + f0 + f] = (float)log(acc > mel_floor ? acc : mel_floor);
    }
}

// ---------------------------------------------------------------------------
// Reflect padding + unfold: y[b][ci * K + j][l] = x[b][c0 + ci][r] (+ x2[b][c02 + ci][r]), r = reflect(l + j * dil - p) at the
// clip's own length L_b, p = dil * (K - 1) / 2; zero for l >= L_b (every column of the pitch is written).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) spk_unfold_kernel(const float* __restrict__ x, int Cx, int c0, const float* __restrict__ x2, int Cx2,
                                                         int c02, const int* __restrict__ n_f, float* __restrict__ y, int C, int K,
                                                         int dil, int ld) {
    const int l = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y, b = blockIdx.z;
    if (l >= ld) return;
    const int ci = r / K, j = r - ci * K, L = n_f[b];
    float v = 0.f;
    if (l < L) {
        const int src = spk_reflect(l + j * dil - dil * (K - 1) / 2, L);
        v = x[((size_t)b * Cx + c0 + ci) * ld + src];
        if (x2) v = v + x2[((size_t)b * Cx2 + c02 + ci) * ld + src];
    }
    y[((size_t)b * C * K + r) * ld + l] = v;
}

// y[b][c0y + c][l] = relu?(x[b][c0x + c][l]) for every column of the pitch
__global__ void __launch_bounds__(256) spk_place_kernel(const float* __restrict__ x, int Cx, int c0x, float* __restrict__ y, int Cy, int c0y,
                                                        int ld, int relu) {
    const int l = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
    if (l >= ld) return;
    float v = x[((size_t)b * Cx + c0x + c) * ld + l];
    if (relu) v = fmaxf(v, 0.f);
    y[((size_t)b * Cy + c0y + c) * ld + l] = v;
}

// one wave per (clip, channel): the mean over the clip's own columns (sum / L, torch's mean)
__global__ void __launch_bounds__(256) spk_rowmean_kernel(const float* __restrict__ x, int C, int ld, const int* __restrict__ n_f,
                                                          float* __restrict__ out) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    if (c >= C) return;   // (a whole wave)
    const int L = n_f[b];
    const float* xr = x + ((size_t)b * C + c) * ld;
    float s = 0.f;
    for (int l = lane; l < L; l += 64) s += xr[l];
    s = wave_sum(s);
    if (lane == 0) out[(size_t)b * C + c] = s / (float)L;
}

// one wave per (clip, output): out[b][o] = act(bias[o] + sum_i w[o][i] in[b][i]); act 0 none, 1 ReLU, 2 sigmoid
__global__ void __launch_bounds__(256) spk_matvec_kernel(const float* __restrict__ w, const float* __restrict__ bias,
                                                         const float* __restrict__ in, float* __restrict__ out, int I, int O, int act) {
    const int lane = threadIdx.x & 63, o = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    if (o >= O) return;
    const float* wr = w + (size_t)o * I;
    const float* xr = in + (size_t)b * I;
    float s = 0.f;
    for (int i = lane; i < I; i += 64) s = fmaf(wr[i], xr[i], s);
    s = wave_sum(s);
    if (lane == 0) {
        float v = s + (bias ? bias[o] : 0.f);
        if (act == 1) v = fmaxf(v, 0.f);
        if (act == 2) v = 1.f / (1.f + expf(-v));
        out[(size_t)b * O + o] = v;
    }
}

// squeeze-excitation's end: v = h[b][c][l] * gate[b][c] + res[b][c][l], to the next block's input y1 [B][C][ld] and to the
// aggregate's slice y2 [B][Cy2][ld] at channel c02
__global__ void __launch_bounds__(256) spk_se_apply_kernel(const float* __restrict__ h, const float* __restrict__ gate,
                                                           const float* __restrict__ res, float* __restrict__ y1, float* __restrict__ y2,
                                                           int Cy2, int c02, int C, int ld) {
    const int l = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
    if (l >= ld) return;
    const size_t i = ((size_t)b * C + c) * ld + l;
    const float v = h[i] * gate[(size_t)b * C + c] + res[i];
    y1[i] = v;
    y2[((size_t)b * Cy2 + c02 + c) * ld + l] = v;
}

// one wave per (clip, channel): mean = sum m x, std = sqrt(max(sum m (x - mean)^2, 1e-12)), m = 1 / L -- two passes
__global__ void __launch_bounds__(256) spk_rowstat_kernel(const float* __restrict__ x, int C, int ld, const int* __restrict__ n_f,
                                                          float* __restrict__ stat) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    if (c >= C) return;
    const int L = n_f[b];
    const float m = 1.f / (float)L;
    const float* xr = x + ((size_t)b * C + c) * ld;
    float s = 0.f;
    for (int l = lane; l < L; l += 64) s = fmaf(m, xr[l], s);
    const float mean = wave_sum(s);
    float q = 0.f;
    for (int l = lane; l < L; l += 64) {
        const float d = xr[l] - mean;
        q = fmaf(m, d * d, q);
    }
    q = wave_sum(q);
    if (lane == 0) {
        stat[(size_t)b * 2 * C + c] = mean;
        stat[(size_t)b * 2 * C + C + c] = sqrtf(fmaxf(q, 1e-12f));
    }
}

// y = tanh(relu(x + bias[b][c])): the class applies both
__global__ void __launch_bounds__(256) spk_att_act_kernel(const float* __restrict__ x, const float* __restrict__ bias, float* __restrict__ y,
                                                          int C, int ld) {
    const int l = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
    if (l >= ld) return;
    const size_t i = ((size_t)b * C + c) * ld + l;
    y[i] = tanhf(fmaxf(x[i] + bias[(size_t)b * C + c], 0.f));
}

// one wave per (clip, channel): a = softmax of z over the clip's own columns; mean = sum a x; std = sqrt(max(sum a (x - mean)^2, 1e-12))
__global__ void __launch_bounds__(256) spk_attnpool_kernel(const float* __restrict__ z, const float* __restrict__ x, int C, int ld,
                                                           const int* __restrict__ n_f, float* __restrict__ pooled) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    if (c >= C) return;
    const int L = n_f[b];
    const float* zr = z + ((size_t)b * C + c) * ld;
    const float* xr = x + ((size_t)b * C + c) * ld;
    float mx = -INFINITY;
    for (int l = lane; l < L; l += 64) mx = fmaxf(mx, zr[l]);
    mx = wave_max(mx);
    float den = 0.f;
    for (int l = lane; l < L; l += 64) den += expf(zr[l] - mx);
    den = wave_sum(den);
    float s = 0.f;
    for (int l = lane; l < L; l += 64) s = fmaf(expf(zr[l] - mx) / den, xr[l], s);
    const float mean = wave_sum(s);
    float q = 0.f;
    for (int l = lane; l < L; l += 64) {
        const float d = xr[l] - mean;
        q = fmaf(expf(zr[l] - mx) / den, d * d, q);
    }
    q = wave_sum(q);
    if (lane == 0) {
        pooled[(size_t)b * 2 * C + c] = mean;
        pooled[(size_t)b * 2 * C + C + c] = sqrtf(fmaxf(q, 1e-12f));
    }
}

// ---------------------------------------------------------------------------
// the launchers: the grid of every kernel above, for the walk and for the one-op test hooks (q3_test_api.hip)
// ---------------------------------------------------------------------------
static inline dim3 spk_cols(int ld, int rows, int B) { return dim3((unsigned)((ld + 255) / 256), (unsigned)rows, (unsigned)B); }
static inline dim3 spk_waves(int rows, int B) { return dim3((unsigned)((rows + 3) / 4), (unsigned)B); }

int spk_launch_unfold(hipStream_t s, const float* x, int Cx, int c0, const float* x2, int Cx2, int c02, const int* n_f, float* y, int C,
                      int K, int dil, int ld, int B) {
    hipLaunchKernelGGL(spk_unfold_kernel, spk_cols(ld, C * K, B), dim3(256), 0, s, x, Cx, c0, x2, Cx2, c02, n_f, y, C, K, dil, ld);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}
int spk_launch_place(hipStream_t s, const float* x, int Cx, int c0x, float* y, int Cy, int c0y, int C, int ld, int relu, int B) {
    hipLaunchKernelGGL(spk_place_kernel, spk_cols(ld, C, B), dim3(256), 0, s, x, Cx, c0x, y, Cy, c0y, ld, relu);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}
int spk_launch_rowmean(hipStream_t s, const float* x, int C, int ld, const int* n_f, float* out, int B) {
    hipLaunchKernelGGL(spk_rowmean_kernel, spk_waves(C, B), dim3(256), 0, s, x, C, ld, n_f, out);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}
int spk_launch_matvec(hipStream_t s, const float* w, const float* bias, const float* in, float* out, int I, int O, int act, int B) {
    hipLaunchKernelGGL(spk_matvec_kernel, spk_waves(O, B), dim3(256), 0, s, w, bias, in, out, I, O, act);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}
int spk_launch_se_apply(hipStream_t s, const float* h, const float* gate, const float* res, float* y1, float* y2, int Cy2, int c02, int C,
                        int ld, int B) {
    hipLaunchKernelGGL(spk_se_apply_kernel, spk_cols(ld, C, B), dim3(256), 0, s, h, gate, res, y1, y2, Cy2, c02, C, ld);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}
int spk_launch_rowstat(hipStream_t s, const float* x, int C, int ld, const int* n_f, float* stat, int B) {
    hipLaunchKernelGGL(spk_rowstat_kernel, spk_waves(C, B), dim3(256), 0, s, x, C, ld, n_f, stat);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}
int spk_launch_att_act(hipStream_t s, const float* x, const float* bias, float* y, int C, int ld, int B) {
    hipLaunchKernelGGL(spk_att_act_kernel, spk_cols(ld, C, B), dim3(256), 0, s, x, bias, y, C, ld);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}
int spk_launch_attnpool(hipStream_t s, const float* z, const float* x, int C, int ld, const int* n_f, float* pooled, int B) {
    hipLaunchKernelGGL(spk_attnpool_kernel, spk_waves(C, B), dim3(256), 0, s, z, x, C, ld, n_f, pooled);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

// ---------------------------------------------------------------------------
// the walk
// ---------------------------------------------------------------------------
struct SpkWalk {
    Spk* e;
    int B, L, ld, launches = 0;
    const int* d_f;   // per-clip frames
    int conv1(const SpkConv& c, const float* x, float* y, bool bias) {
        ConvArgs a;
        a.Cin = c.cin * c.k;
        a.K = 1;
        a.dil = 1;
        a.wk = c.w;
        a.bias = bias ? c.b : nullptr;
        a.Cout = a.M = c.cout;
        a.stride = 1;
        a.Lin = a.Lout = a.Lc = L;
        a.Lrule = 1 << 20;   // never the short-activation variants: the rule depends on nothing in the call (enc_conv_args)
        a.ldx = a.ldy = ld;
        a.x = x;
        a.y = y;
        launches++;
        return voc_launch_conv(e->s, a, B, e->cfg);
    }
    int unfold(const SpkConv& c, const float* x, int Cx, int c0, const float* x2, int Cx2, int c02) {
        launches++;
        return spk_launch_unfold(e->s, x, Cx, c0, x2, Cx2, c02, d_f, e->unf, c.cin, c.k, c.dil, ld, B);
    }
    int place(const float* x, int Cx, int c0x, float* y, int Cy, int c0y, int C, int relu) {
        launches++;
        return spk_launch_place(e->s, x, Cx, c0x, y, Cy, c0y, C, ld, relu, B);
    }
    // relu(conv(x)) of channels [c0, c0 + cin) of x (+ x2's), into channels [c0y, c0y + cout) of y
    int tdnn(const SpkConv& c, const float* x, int Cx, int c0, const float* x2, int Cx2, int c02, float* y, int Cy, int c0y) {
        const float* in = x;
        if (c.k != 1 || c0 != 0 || Cx != c.cin || x2) {
            if (unfold(c, x, Cx, c0, x2, Cx2, c02)) return -1;
            in = e->unf;
        }
        if (conv1(c, in, e->raw, true)) return -1;
        return place(e->raw, c.cout, 0, y, Cy, c0y, c.cout, 1);
    }
    int matvec(const SpkLin& m, const float* in, float* out, int act) {
        launches++;
        return spk_launch_matvec(e->s, m.w, m.b, in, out, m.in, m.out, act, B);
    }
};

// Runs the walk on the B clips in e->pcm up to and including `stage` (0 block0, 1..nb the SE-Res2Net blocks, nb + 1 mfa,
// nb + 2 asp, nb + 3 fc; < 0: the log-mel only).  -> where that stage's output is: buffer, its channels per clip, the first
// channel, the channels of the stage, and whether it is pooled ([B][C] instead of [B][C][ld]).
struct SpkOut {
    const float* p = nullptr;
    int Ctot = 0, c0 = 0, C = 0, pooled = 0;
};
static int spk_run(Spk* e, int B, const std::vector<int>& ns, const std::vector<int>& fs, int stage, SpkOut* o) {
    const int L = *std::max_element(fs.begin(), fs.begin() + B);
    const int Ls = *std::max_element(ns.begin(), ns.begin() + B);
    SpkWalk w{e, B, L, (int)spk_pitch(L)};
    w.d_f = e->d_n + e->max_batch;
    e->run_B = B;
    e->run_L = L;
    e->run_ld = w.ld;
    e->last_launches = 0;
    const int nb = (int)e->blocks.size();
    {
        const size_t lds = (size_t)(SPK_FT + 2) * e->n_fft * sizeof(double);
        hipLaunchKernelGGL(spk_mel_kernel, dim3((unsigned)((L + SPK_FT - 1) / SPK_FT), (unsigned)B), dim3(256), lds, e->s, e->pcm,
                           (int)spk_pitch(Ls), e->d_n, w.d_f, e->d_win, e->d_cos, e->d_sin, e->d_fb, e->mel, w.ld, e->n_fft, e->hop, e->pad,
                           e->n_mels, e->mel_floor, e->mag_eps);
        w.launches++;
        Q3_HIP(hipGetLastError(), -1);
    }
    auto done = [&](const float* p, int Ctot, int c0, int C, int pooled) {
        *o = SpkOut{p, Ctot, c0, C, pooled};
        e->last_launches = w.launches;
        return 0;
    };
    if (stage < 0) return done(e->mel, e->n_mels, 0, e->n_mels, 0);
    const int C = e->C, Cm = e->Cm, cw = C / e->scale;
    float* cur = e->xo[0];
    if (w.tdnn(e->block0, e->mel, e->n_mels, 0, nullptr, 0, 0, cur, C, 0)) return -1;
    if (stage == 0) return done(cur, C, 0, C, 0);
    for (int i = 0; i < nb; i++) {
        const SpkBlock& k = e->blocks[i];
        float* nxt = e->xo[(i + 1) & 1];
        if (w.tdnn(k.tdnn1, cur, C, 0, nullptr, 0, 0, e->h1, C, 0)) return -1;
        if (w.place(e->h1, C, 0, e->r2, C, 0, cw, 0)) return -1;   // chunk 0 passes through
        for (int j = 1; j < e->scale; j++)                          // chunk 1: conv(chunk); chunk j >= 2: conv(chunk_j + out_{j-1})
            if (w.tdnn(k.res[j - 1], e->h1, C, j * cw, j >= 2 ? e->r2 : nullptr, C, (j - 1) * cw, e->r2, C, j * cw)) return -1;
        if (w.tdnn(k.tdnn2, e->r2, C, 0, nullptr, 0, 0, e->h2, C, 0)) return -1;
        w.launches++;
        if (spk_launch_rowmean(e->s, e->h2, C, w.ld, w.d_f, e->semean, B)) return -1;
        if (w.matvec(k.se1, e->semean, e->sehid, 1) || w.matvec(k.se2, e->sehid, e->gate, 2)) return -1;
        w.launches++;
        if (spk_launch_se_apply(e->s, e->h2, e->gate, cur, nxt, e->cat, Cm, i * C, C, w.ld, B)) return -1;
        cur = nxt;
        if (stage == i + 1) return done(cur, C, 0, C, 0);
    }
    if (w.tdnn(e->mfa, e->cat, Cm, 0, nullptr, 0, 0, e->xm, Cm, 0)) return -1;
    if (stage == nb + 1) return done(e->xm, Cm, 0, Cm, 0);
    w.launches++;
    if (spk_launch_rowstat(e->s, e->xm, Cm, w.ld, w.d_f, e->stat, B)) return -1;
    if (w.matvec(e->asp_stat, e->stat, e->abias, 0)) return -1;
    if (w.conv1(e->asp_tdnn, e->xm, e->raw, false)) return -1;
    const int A = e->asp_tdnn.cout;
    w.launches++;
    if (spk_launch_att_act(e->s, e->raw, e->abias, e->att, A, w.ld, B)) return -1;
    if (w.conv1(e->asp_conv, e->att, e->logit, true)) return -1;
    w.launches++;
    if (spk_launch_attnpool(e->s, e->logit, e->xm, Cm, w.ld, w.d_f, e->pooled, B)) return -1;
    if (stage == nb + 2) return done(e->pooled, 2 * Cm, 0, 2 * Cm, 1);
    if (w.matvec(e->fc, e->pooled, e->emb, 0)) return -1;
    return done(e->emb, e->dim, 0, e->dim, 1);
}

static void spk_destroy(Spk* e) {
    if (!e) return;
    if (e->s) hipStreamSynchronize(e->s);
    e->mem.release();
    if (e->e0) hipEventDestroy(e->e0);
    if (e->e1) hipEventDestroy(e->e1);
    if (e->s) hipStreamDestroy(e->s);
    delete e;
}

// checks the arguments and uploads the clips and their lengths -> 0 / <0 (one logged line)
static int spk_upload(Spk* e, const float* pcm, const int32_t* n, int B, std::vector<int>& ns, std::vector<int>& fs, const char* who) {
    if (!pcm || !n) {
        Q3_LOG("%s: NULL pcm or n_samples", who);
        return -1;
    }
    if (B < 1 || B > e->max_batch) {
        Q3_LOG("%s: B = %d outside 1..%d (max_batch)", who, B, e->max_batch);
        return -1;
    }
    ns.assign(e->max_batch, 0);
    fs.assign(e->max_batch, 0);
    size_t total = 0;
    for (int b = 0; b < B; b++) {
        const int f = n[b] > e->max_samples ? -1 : spk_frames_of(e->n_fft, e->hop, e->pad, e->min_frames, n[b]);
        if (f < 0) {
            Q3_LOG("%s: clip %d has %d samples (%d..%d: more than the reflect padding and at least %d frames)", who, b, n[b],
                   spk_min_samples_of(e->n_fft, e->hop, e->pad, e->min_frames), e->max_samples, e->min_frames);
            return -1;
        }
        ns[b] = n[b];
        fs[b] = f;
        total += (size_t)n[b];
    }
    for (size_t i = 0; i < total; i++)
        if (!std::isfinite(pcm[i])) {
            Q3_LOG("%s: sample %zu is not finite", who, i);
            return -1;
        }
    const long ldp = spk_pitch(*std::max_element(ns.begin(), ns.begin() + B));
    size_t off = 0;
    for (int b = 0; b < B; b++) {
        Q3_HIP(hipMemcpyAsync(e->pcm + (size_t)b * ldp, pcm + off, (size_t)n[b] * 4, hipMemcpyHostToDevice, e->s), -1);
        off += (size_t)n[b];
    }
    std::vector<int> tab(ns);
    tab.insert(tab.end(), fs.begin(), fs.end());
    Q3_HIP(hipMemcpyAsync(e->d_n, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, e->s), -1);
    Q3_HIP(hipStreamSynchronize(e->s), -1);   // (tab is a local)
    return 0;
}

static int spk_debug(Spk* e, const float* pcm, const int32_t* n, int B, int stage, float* out, int* C, int* L, const char* who) {
    if (!e || !out || !C || !L) return -1;
    spk_enter(e);
    const int last = (int)e->blocks.size() + 3;
    if (stage > last) {
        Q3_LOG("%s: stage %d past the last (%d)", who, stage, last);
        return -1;
    }
    std::vector<int> ns, fs;
    if (spk_upload(e, pcm, n, B, ns, fs, who)) return -1;
    SpkOut o;
    if (spk_run(e, B, ns, fs, stage, &o)) return -1;
    *C = o.C;
    if (o.pooled) {
        *L = 1;
        Q3_HIP(hipMemcpyAsync(out, o.p, (size_t)B * o.C * 4, hipMemcpyDeviceToHost, e->s), -1);
    } else {
        *L = e->run_L;
        for (int b = 0; b < B; b++)
            Q3_HIP(hipMemcpy2DAsync(out + (size_t)b * o.C * e->run_L, sizeof(float) * (size_t)e->run_L,
                                    o.p + ((size_t)b * o.Ctot + o.c0) * e->run_ld, sizeof(float) * (size_t)e->run_ld,
                                    sizeof(float) * (size_t)e->run_L, (size_t)o.C, hipMemcpyDeviceToHost, e->s), -1);
    }
    Q3_HIP(hipStreamSynchronize(e->s), -1);
    return 0;
}
int spk_debug_mel(Spk* e, const float* pcm, const int32_t* n, int B, float* out, int* C, int* L) {
    return spk_debug(e, pcm, n, B, -1, out, C, L, "spk mel hook");
}
int spk_debug_stage(Spk* e, const float* pcm, const int32_t* n, int B, int stage, float* out, int* C, int* L) {
    if (stage < 0) return -1;
    return spk_debug(e, pcm, n, B, stage, out, C, L, "spk stage hook");
}

}  // namespace q3

using namespace q3;

extern "C" {

void spk_free(void* h) {
    spk_enter((Spk*)h);
    spk_destroy((Spk*)h);
}

void* spk_load(const char* weights, int max_batch, int max_samples) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        Q3_LOG("no HIP device available -- this library has no CPU path");
        return nullptr;
    }
    if (!weights || max_batch <= 0 || max_samples <= 0) {
        Q3_LOG("spk_load: needs a weight file, max_batch > 0 and max_samples > 0");
        return nullptr;
    }
    Pack p;
    if (!p.open(weights)) return nullptr;
    const PackTensor* geo = p.find("spk.geometry");
    if (!geo || geo->dtype != I32 || geo->ndim != 2 || geo->shape[0] != 3 || geo->shape[1] < 3 || geo->shape[1] > 16) {
        Q3_LOG("%s holds no speaker encoder (tensor spk.geometry int32 [3][blocks]: channels, kernel sizes, dilations)", weights);
        return nullptr;
    }
    Spk* e = new Spk();
    hipGetDevice(&e->device);
    e->max_batch = max_batch;
    e->max_samples = max_samples;
    e->sample_rate = (int)p.get("spk_sample_rate", 24000);
    e->n_fft = (int)p.get("spk_n_fft", 0);
    e->hop = (int)p.get("spk_hop", 0);
    e->pad = (int)p.get("spk_pad", -1);
    e->n_mels = (int)p.get("spk_n_mels", 0);
    e->mel_floor = p.get("spk_mel_floor", 1e-5);
    e->mag_eps = p.get("spk_mag_eps", 1e-9);
    e->scale = (int)p.get("spk_res2net_scale", 0);
    e->dim = (int)p.get("spk_dim", 0);
    const int win = (int)p.get("spk_win", 0), se = (int)p.get("spk_se_channels", 0), A = (int)p.get("spk_attention_channels", 0);
    const int nblk = (int)geo->shape[1], nb = nblk - 2;
    const int32_t* g = (const int32_t*)geo->data;
    const int32_t *gc = g, *gk = g + nblk, *gd = g + 2 * nblk;
    bool ok = true;
    auto fail = [&](const char* why) {
        if (ok) Q3_LOG("spk_load: %s", why);
        ok = false;
    };
    if (e->n_fft < 8 || e->n_fft > 1024 || (e->n_fft & 1) || win != e->n_fft || e->hop < 1 || e->pad < 0 || e->pad >= e->n_fft || e->n_mels < 8 ||
        e->n_mels > 1024 || !(e->mel_floor > 0.0) || !(e->mag_eps >= 0.0) || e->sample_rate <= 0)
        fail("mel parameters (even n_fft <= 1024 = win, hop >= 1, 0 <= pad < n_fft, 8 <= n_mels <= 1024, mel_floor > 0)");
    e->C = gc[0];
    e->Cm = gc[nblk - 1];
    int maxp = 0;
    long sum = 0;
    for (int i = 0; i < nblk && ok; i++) {
        if (gc[i] <= 0 || gc[i] > 8192 || gk[i] < 1 || gk[i] > 15 || !(gk[i] & 1) || gd[i] < 1 || gd[i] > 64) fail("block geometry (odd kernel sizes <= 15, dilations <= 64)");
        if (i < nblk - 1 && gc[i] != e->C) fail("the blocks before the aggregation share one width (the SE blocks add their input)");
        if (i >= 1 && i < nblk - 1) sum += gc[i];
        maxp = std::max(maxp, gd[i] * (gk[i] - 1) / 2);
    }
    if (ok && (sum != e->Cm)) fail("the aggregation's width is the sum of the SE blocks' widths");
    if (ok && (e->scale < 2 || e->C % e->scale || (e->C / e->scale) % 8 || e->C % 8 || e->Cm % 8 || (e->n_mels * gk[0]) % 8 || se < 1 || A < 8 || A % 8 ||
               e->dim < 1))
        fail("widths (C / scale, C, the aggregate, n_mels * k0 and the attention width are multiples of 8)");
    e->min_frames = maxp + 1;
    e->max_frames = ok ? spk_frames_of(e->n_fft, e->hop, e->pad, e->min_frames, max_samples) : -1;
    if (ok && e->max_frames < 0) fail("max_samples is below the shortest clip the geometry takes");
    ok = ok && hipStreamCreateWithFlags(&e->s, hipStreamNonBlocking) == hipSuccess && hipEventCreate(&e->e0) == hipSuccess &&
         hipEventCreate(&e->e1) == hipSuccess;
    auto up = [&](const std::string& name, uint64_t ne) -> float* {
        if (!ok) return nullptr;
        const PackTensor* t = p.find(name);
        if (!t || t->dtype != F32 || t->numel() != ne) {
            Q3_LOG("spk_load: tensor %s missing or not f32 with %llu elements", name.c_str(), (unsigned long long)ne);
            ok = false;
            return nullptr;
        }
        const float* h = (const float*)t->data;
        for (uint64_t i = 0; i < ne; i++)
            if (!std::isfinite(h[i])) {
                Q3_LOG("spk_load: tensor %s holds a non-finite value", name.c_str());
                ok = false;
                return nullptr;
            }
        float* d = nullptr;
        if (!e->mem.alloc(&d, ne * 4) || hipMemcpy(d, h, ne * 4, hipMemcpyHostToDevice) != hipSuccess) {
            Q3_LOG("spk_load: no device memory for %s", name.c_str());
            ok = false;
            return nullptr;
        }
        return d;
    };
    auto conv = [&](const std::string& base, int cin, int cout, int k, int dil, bool bias) {
        SpkConv c;
        c.cin = cin;
        c.cout = cout;
        c.k = k;
        c.dil = dil;
        c.w = up(base + ".w", (uint64_t)cin * k * ((cout + 3) / 4 * 4));
        c.b = bias ? up(base + ".b", (uint64_t)cout) : nullptr;
        return c;
    };
    auto lin = [&](const std::string& base, int in, int out, const std::string& bias) {
        SpkLin m;
        m.in = in;
        m.out = out;
        m.w = up(base, (uint64_t)in * out);
        m.b = up(bias, (uint64_t)out);
        return m;
    };
    if (ok) {
        const int C = e->C, Cm = e->Cm, cw = C / e->scale;
        e->block0 = conv("spk.block0", e->n_mels, C, gk[0], gd[0], true);
        for (int i = 1; i <= nb && ok; i++) {
            const std::string b = "spk.block" + std::to_string(i);
            SpkBlock k;
            k.tdnn1 = conv(b + ".tdnn1", C, C, 1, 1, true);
            for (int j = 0; j < e->scale - 1; j++) k.res.push_back(conv(b + ".res" + std::to_string(j), cw, cw, gk[i], gd[i], true));
            k.tdnn2 = conv(b + ".tdnn2", C, C, 1, 1, true);
            k.se1 = lin(b + ".se1.w", C, se, b + ".se1.b");
            k.se2 = lin(b + ".se2.w", se, C, b + ".se2.b");
            e->blocks.push_back(k);
        }
        e->mfa = conv("spk.mfa", Cm, Cm, gk[nblk - 1], gd[nblk - 1], true);
        e->asp_tdnn = conv("spk.asp.tdnn", Cm, A, 1, 1, false);
        e->asp_stat = lin("spk.asp.tdnn.wstat", 2 * Cm, A, "spk.asp.tdnn.b");
        e->asp_conv = conv("spk.asp.conv", A, Cm, 1, 1, true);
        e->fc = lin("spk.fc.w", 2 * Cm, e->dim, "spk.fc.b");
    }
    // the front-end's tables: the filter bank as stored (f64 bit patterns in an int64 tensor: the container has no f64
    // type), the periodic Hann window and the twiddles in double
    const int NB = e->n_fft / 2 + 1;
    if (ok) {
        const PackTensor* fb = p.find("spk.mel_fb");
        if (!fb || fb->dtype != I64 || fb->ndim != 2 || (int)fb->shape[0] != NB || (int)fb->shape[1] != e->n_mels) {
            fail("tensor spk.mel_fb (the f64 filter bank [n_fft / 2 + 1][n_mels], stored as int64 bit patterns) missing or misshapen");
        } else {
            const size_t ne = (size_t)NB * e->n_mels;
            std::vector<double> h(ne);
            memcpy(h.data(), fb->data, ne * 8);
            for (size_t i = 0; i < ne && ok; i++)
                if (!std::isfinite(h[i])) fail("non-finite filter-bank entry");
            std::vector<double> wn(e->n_fft), cs(e->n_fft), sn(e->n_fft);
            const double PI = 3.14159265358979323846;
            for (int j = 0; j < e->n_fft; j++) {
                wn[j] = 0.5 - 0.5 * std::cos(2.0 * PI * j / e->n_fft);
                cs[j] = std::cos(2.0 * PI * j / e->n_fft);
                sn[j] = std::sin(2.0 * PI * j / e->n_fft);
            }
            auto upd = [&](double** d, const std::vector<double>& v) {
                return e->mem.alloc(d, v.size() * 8) && hipMemcpy(*d, v.data(), v.size() * 8, hipMemcpyHostToDevice) == hipSuccess;
            };
            if (ok && !(upd(&e->d_fb, h) && upd(&e->d_win, wn) && upd(&e->d_cos, cs) && upd(&e->d_sin, sn))) fail("no device memory for the mel tables");
        }
    }
    if (ok) {
        const size_t ld = (size_t)spk_pitch(e->max_frames), Bz = (size_t)max_batch;
        const int C = e->C, Cm = e->Cm, cw = C / e->scale;
        size_t unf_rows = (size_t)e->n_mels * gk[0];
        for (int i = 1; i <= nb; i++) unf_rows = std::max(unf_rows, (size_t)cw * gk[i]);
        unf_rows = std::max(unf_rows, (size_t)std::max(C, Cm) * (size_t)std::max(1, (int)gk[nblk - 1]));
        const size_t big = std::max(unf_rows, (size_t)std::max(std::max(C, Cm), e->n_mels));
        if (Bz * big * ld >= ((size_t)1 << 31) || Bz * (size_t)spk_pitch(max_samples) >= ((size_t)1 << 31) || big > 65535 || Bz > 65535) {
            fail("clips this many and this long are beyond the kernels' 32-bit indexing");
        } else {
            auto z = [&](float** d, size_t n) { ok = ok && e->mem.alloc_zeroed(d, n * 4, e->s); };   // (zeroed once: pad columns start finite)
            z(&e->pcm, Bz * spk_pitch(max_samples));
            z(&e->mel, Bz * e->n_mels * ld);
            z(&e->unf, Bz * unf_rows * ld);
            z(&e->raw, Bz * std::max(std::max(C, Cm), A) * ld);
            z(&e->xo[0], Bz * C * ld);
            z(&e->xo[1], Bz * C * ld);
            z(&e->h1, Bz * C * ld);
            z(&e->r2, Bz * C * ld);
            z(&e->h2, Bz * C * ld);
            z(&e->cat, Bz * Cm * ld);
            z(&e->xm, Bz * Cm * ld);
            z(&e->att, Bz * A * ld);
            z(&e->logit, Bz * Cm * ld);
            z(&e->semean, Bz * C);
            z(&e->sehid, Bz * se);
            z(&e->gate, Bz * C);
            z(&e->stat, Bz * 2 * Cm);
            z(&e->abias, Bz * A);
            z(&e->pooled, Bz * 2 * Cm);
            z(&e->emb, Bz * e->dim);
            ok = ok && e->mem.alloc(&e->d_n, 2 * Bz * sizeof(int)) && hipDeviceSynchronize() == hipSuccess;
            if (!ok) Q3_LOG("spk_load: no device memory for %d clips of %d samples", max_batch, max_samples);
        }
    }
    if (!ok) {
        Q3_LOG("spk_load failed");
        spk_destroy(e);
        return nullptr;
    }
    return e;
}

int spk_dim(void* h) { return h ? ((Spk*)h)->dim : 0; }
int spk_sample_rate(void* h) { return h ? ((Spk*)h)->sample_rate : 0; }
int spk_min_samples(void* h) {
    Spk* e = (Spk*)h;
    return e ? spk_min_samples_of(e->n_fft, e->hop, e->pad, e->min_frames) : 0;
}
int spk_frames(void* h, int n) {
    Spk* e = (Spk*)h;
    return e ? spk_frames_of(e->n_fft, e->hop, e->pad, e->min_frames, n) : -1;
}
float spk_last_ms(void* h) { return h ? ((Spk*)h)->last_ms : -1.f; }
int spk_last_launches(void* h) { return h ? ((Spk*)h)->last_launches : -1; }

int spk_embed(void* h, const float* pcm, const int32_t* n_samples, int B, float* out) {
    Spk* e = (Spk*)h;
    if (!e) {
        Q3_LOG("spk_embed: NULL handle");
        return -1;
    }
    spk_enter(e);
    if (!out) {
        Q3_LOG("spk_embed: NULL out");
        return -1;
    }
    std::vector<int> ns, fs;
    Q3_HIP(hipEventRecord(e->e0, e->s), -1);
    if (spk_upload(e, pcm, n_samples, B, ns, fs, "spk_embed")) return -1;
    SpkOut o;
    if (spk_run(e, B, ns, fs, (int)e->blocks.size() + 3, &o)) return -1;
    Q3_HIP(hipMemcpyAsync(out, e->emb, (size_t)B * e->dim * 4, hipMemcpyDeviceToHost, e->s), -1);
    Q3_HIP(hipEventRecord(e->e1, e->s), -1);
    Q3_HIP(hipStreamSynchronize(e->s), -1);
    hipEventElapsedTime(&e->last_ms, e->e0, e->e1);
    return 0;
}

}  // extern "C"
