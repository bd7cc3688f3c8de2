// q3_spk.h -- the speaker encoder's host arithmetic (no device call: tests/spk_host_driver.cpp compiles it as it stands)
// and the handle q3_spk.hip and the test library share.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define Q3_SPK_HD __host__ __device__
#else
#define Q3_SPK_HD
#endif

namespace q3 {

// Frames of a clip of n samples: the clip is reflect-padded by `pad` at both ends, frame f covers padded samples
// [f * hop, f * hop + n_fft).  < 0: the reflection needs n > pad, and the network's widest reflect padding needs
// min_frames columns (dilation 4 at 3 taps: padding 4 on at least 5 columns).
static inline int spk_frames_of(int n_fft, int hop, int pad, int min_frames, long long n) {
    if (n_fft <= 0 || hop <= 0 || pad < 0 || n <= pad) return -1;
    const long long span = n + 2LL * pad - n_fft;
    if (span < 0) return -1;
    const long long f = 1 + span / hop;
    if (f < min_frames || f > 0x7fffffffLL) return -1;
    return (int)f;
}
// the shortest clip spk_frames_of accepts
static inline int spk_min_samples_of(int n_fft, int hop, int pad, int min_frames) {
    long long n = (long long)(min_frames - 1) * hop + n_fft - 2LL * pad;
    if (n < pad + 1) n = pad + 1;
    return (int)n;
}
// column l of a row of L columns under "same" reflect padding: index l + off, reflected at the row's own ends (|off| < L)
Q3_SPK_HD static inline int spk_reflect(int i, int L) { return i < 0 ? -i : (i >= L ? 2 * (L - 1) - i : i); }

}  // namespace q3

#ifdef __HIPCC__
#include "q3_common.h"
#include "q3_voc_ops.h"

#include <vector>

namespace q3 {

// a conv as the exact-f32 launcher runs it: ONE tap over the cin * k rows the reflect-unfold kernel writes
struct SpkConv {
    float *w = nullptr, *b = nullptr;   // w: conv_kernel's packed layout [cin * k / 8][1][8][Mp]
    int cin = 0, cout = 0, k = 1, dil = 1;
};
// a matvec over per-clip vectors: w plain [out][in]
struct SpkLin {
    float *w = nullptr, *b = nullptr;
    int in = 0, out = 0;
};
struct SpkBlock {
    SpkConv tdnn1, tdnn2;
    std::vector<SpkConv> res;   // scale - 1 convs over C / scale channels
    SpkLin se1, se2;
};

struct Spk {
    int device = 0, max_batch = 1, max_samples = 0, max_frames = 0, min_frames = 5;
    VocSettings cfg;   // the call's snapshot of the process-wide settings (spk_enter): voc_launch_conv's grid cap and fill
    int sample_rate = 24000, n_fft = 1024, hop = 256, pad = 384, n_mels = 128;
    double mel_floor = 1e-5, mag_eps = 1e-9;
    int C = 0, Cm = 0, scale = 8, dim = 0;   // block width, aggregated width (the SE blocks' outputs side by side)
    double *d_win = nullptr, *d_cos = nullptr, *d_sin = nullptr, *d_fb = nullptr;
    SpkConv block0, mfa, asp_tdnn, asp_conv;
    SpkLin asp_stat, fc;   // asp_stat: the [mean; std] columns of asp.tdnn as a per-clip bias
    std::vector<SpkBlock> blocks;
    DeviceAllocs mem;
    hipStream_t s = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    float* pcm = nullptr;      // [max_batch][pitch(max_samples)]
    int* d_n = nullptr;        // [2][max_batch]: samples, frames
    float *mel = nullptr, *unf = nullptr, *raw = nullptr, *xo[2] = {nullptr, nullptr}, *h1 = nullptr, *r2 = nullptr, *h2 = nullptr, *cat = nullptr,
          *xm = nullptr, *att = nullptr, *logit = nullptr;
    float *semean = nullptr, *sehid = nullptr, *gate = nullptr, *stat = nullptr, *abias = nullptr, *pooled = nullptr, *emb = nullptr;
    float last_ms = 0.f;
    int last_launches = 0;
    // of the last run: what the stage hooks read back
    int run_B = 0, run_L = 0, run_ld = 0;
};

// every entry point that touches the GPU: binds the thread to the handle's device and takes the call's one settings snapshot
static inline void spk_enter(Spk* e) {
    if (!e) return;
    int d = -1;
    if (hipGetDevice(&d) != hipSuccess || d != e->device) hipSetDevice(e->device);
    e->cfg = voc_settings.load();
}

// rows are [clip][channel] at a pitch of the call's longest clip's frames rounded up to 32 floats
static inline long spk_pitch(long L) { return (L + 31) & ~31L; }

// One launch of each of the network's own kernels (q3_spk.hip states them), on B clips of pitch ld whose frame counts are
// n_f [B] on the device: the walk's grids, shared with the one-op test hooks (q3t_spk_*_case).  0 / <0.
// y [B][C * K][ld] = reflect-unfold of channels [c0, c0 + C) of x [B][Cx][ld] (+ channels [c02, c02 + C) of x2 [B][Cx2][ld])
int spk_launch_unfold(hipStream_t s, const float* x, int Cx, int c0, const float* x2, int Cx2, int c02, const int* n_f, float* y, int C,
                      int K, int dil, int ld, int B);
// channels [c0y, c0y + C) of y [B][Cy][ld] = relu?(channels [c0x, c0x + C) of x [B][Cx][ld]), every column of the pitch
int spk_launch_place(hipStream_t s, const float* x, int Cx, int c0x, float* y, int Cy, int c0y, int C, int ld, int relu, int B);
// out [B][C] = the mean of x [B][C][ld] over the clip's own columns
int spk_launch_rowmean(hipStream_t s, const float* x, int C, int ld, const int* n_f, float* out, int B);
// out [B][O] = act(bias + w [O][I] in [B][I]); bias may be null; act 0 none, 1 ReLU, 2 sigmoid
int spk_launch_matvec(hipStream_t s, const float* w, const float* bias, const float* in, float* out, int I, int O, int act, int B);
// y1 [B][C][ld] and channels [c02, c02 + C) of y2 [B][Cy2][ld] = h * gate [B][C] + res, every column of the pitch
int spk_launch_se_apply(hipStream_t s, const float* h, const float* gate, const float* res, float* y1, float* y2, int Cy2, int c02, int C,
                        int ld, int B);
// stat [B][2 C] = mean | std of x [B][C][ld] over the clip's own columns
int spk_launch_rowstat(hipStream_t s, const float* x, int C, int ld, const int* n_f, float* stat, int B);
// y = tanh(relu(x + bias [B][C])), every column of the pitch
int spk_launch_att_act(hipStream_t s, const float* x, const float* bias, float* y, int C, int ld, int B);
// pooled [B][2 C] = softmax(z)-weighted mean | std of x over the clip's own columns
int spk_launch_attnpool(hipStream_t s, const float* z, const float* x, int C, int ld, const int* n_f, float* pooled, int B);

// test hooks' back ends (q3_test_api.hip wraps them as q3t_spk_mel / q3t_spk_stage): run spk_embed's walk on the clips and
// return the log-mel dense [B][n_mels][L] / the activation after `stage` dense [B][C][L] (L: the longest clip's frames;
// pooled stages: [B][C], L = 1).  Stage 0 block0, 1.. the SE-Res2Net blocks, then mfa, asp, fc.  0 / <0.
int spk_debug_mel(Spk* e, const float* pcm, const int32_t* n_samples, int B, float* out, int* C, int* L);
int spk_debug_stage(Spk* e, const float* pcm, const int32_t* n_samples, int B, int stage, float* out, int* C, int* L);

}  // namespace q3
#endif
