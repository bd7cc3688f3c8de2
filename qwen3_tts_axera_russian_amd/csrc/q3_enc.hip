// q3_enc.hip -- fp32 speech-tokenizer encoder (24 kHz audio -> codec ids) for gfx950, include/qwen3tts_enc.h.
//
// Interprets the op table `enc.program` (int32 [n_ops][8], weights.py enc_program, DESIGN.md "Speech tokenizer
// encoder") whose semantics are pinned to transformers' MimiModel.encode.  Activations are [B][C][ld] f32 with a row
// pitch ld = L rounded up to 32 floats, one row per clip and channel, L = the longest clip's columns at that stage.
//
// Shared with the vocoder (q3_voc_ops.h, defined in q3_voc_kernels.hip): the exact-fp32 MFMA conv (with ELU applied while the input is staged),
// the channel norm and the sliding-window attention; q3_enc.h turns a conv op into the conv launcher's arguments (enc_conv_args)
// for enc_run here and for the streaming walk (q3_enc_stream.hip).  Own kernels:
//   enc_conv_in_kernel   the first conv, ONE input channel (a dot product of k taps per output: no MFMA tile), for a whole clip
//                        and for a stream's push (the k - 1 carried samples left of column 0): enc_launch_conv_in
//   enc_unfold_kernel    strided conv input -> [Cin * k][ceil(L / s)] columns (im2col), Mimi's padding per clip: zeros
//                        (ELU'd, ELU(0) = 0) or replicate at both edges.  The strided conv is then a 1-tap conv.
//   enc_rvq_kernel       split residual VQ encode: per frame, stage q scores ||e_j||^2 - 2 r.e_j for every entry j,
//                        takes the lowest-index arg-min and subtracts e_idx from the residual.
//
// Ragged batches: every op's arithmetic for a column reads only that column and the columns left of it in its own clip
// (causal convs, causal attention), or -- the strided ops -- the clip's own padding substituted for any column at or past
// its own length, so the padding columns of a shorter clip never reach its kept outputs.  No variant rule looks at the
// batch or the lengths (enc_conv_args' pin, ConvArgs::elu, voc_launch_attn): clip b gives the same bits alone and in a batch.
#include "../../include/qwen3tts_enc.h"
#include "q3_enc.h"

#include <algorithm>
#include <cmath>
#include <utility>

namespace q3 {

// ---------------------------------------------------------------------------
// First conv: x [B][ldx] (one channel, n columns) -> y [B][Cout][ldy], causal k taps, + bias.  One thread per column holds its
// k inputs and walks the output channels (weights: wave-uniform loads): bias first, then the taps in order.  Left of column 0
// are zeros (hist == nullptr: a whole clip) or the last K - 1 samples of the entry's stream, which only workgroup 0 reads
// (columns < K - 1) and, after a barrier, replaces with the last K - 1 of [history | new].
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) enc_conv_in_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ y, int ldy,
                                                          int Cout, int K, int n, float* hist, long long state_floats,
                                                          const int* __restrict__ streams) {
    const int l = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y, H = K - 1;
    const float* xb = x + (size_t)b * ldx;
    float* h = hist ? hist + (size_t)streams[b] * state_floats : nullptr;
    float nw = 0.f;
    const bool roll = h && blockIdx.x == 0 && (int)threadIdx.x < H;
    if (roll) nw = ((int)threadIdx.x + n < H) ? h[threadIdx.x + n] : xb[(int)threadIdx.x + n - H];
    if (l < n) {
        float xv[ENC_IN_MAXK];
#pragma unroll
        for (int k = 0; k < ENC_IN_MAXK; k++) {
            const int ls = l - (K - 1 - k);
            xv[k] = k < K ? (ls >= 0 ? xb[ls] : (h ? h[H + ls] : 0.f)) : 0.f;
        }
        float* yb = y + (size_t)b * Cout * ldy + l;
        for (int co = 0; co < Cout; co++) {
            float acc = bias ? bias[co] : 0.f;
#pragma unroll
            for (int k = 0; k < ENC_IN_MAXK; k++)
                if (k < K) acc = fmaf(w[co * K + k], xv[k], acc);
            yb[(size_t)co * ldy] = acc;
        }
    }
    __syncthreads();
    if (roll) h[threadIdx.x] = nw;
}

int enc_launch_conv_in(hipStream_t s, const float* x, int ldx, const EncOp& op, float* y, int ldy, int n, int B, float* hist,
                       long long state_floats, const int* streams) {
    hipLaunchKernelGGL(enc_conv_in_kernel, dim3((unsigned)((n + 255) / 256), B), dim3(256), 0, s, x, ldx, op.w, op.bias, y, ldy, op.cout,
                       op.k, n, hist, state_floats, streams);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

// ---------------------------------------------------------------------------
// Strided conv input (MimiConv1d, stride s, k taps, padding_total = k - s on the left, the right padded to whole
// frames): y[b][ci * k + j][u] = act(xpad_b[u * s + j - (k - s)]) for u < ceil(len_b / s), 0 after that, where
// xpad_b is clip b's row with its own padding for every index < 0 or >= len_b: zero, or (replicate) x[0] / x[len_b - 1].
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) enc_unfold_kernel(const float* __restrict__ x, int ldx, int Cin, const int* __restrict__ lens,
                                                         float* __restrict__ y, int ldy, int Lout, int k, int s, int replicate,
                                                         int elu) {
    const int u = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y, b = blockIdx.z;
    if (u >= Lout) return;
    const int ci = r / k, j = r - ci * k;
    const int len = lens[b];
    const int nout = (len + s - 1) / s;
    float v = 0.f;
    if (u < nout) {
        int i = u * s + j - (k - s);
        const float* xr = x + ((size_t)b * Cin + ci) * ldx;
        if (replicate) {
            i = i < 0 ? 0 : (i >= len ? len - 1 : i);
            v = xr[i];
        } else if (i >= 0 && i < len) {
            v = xr[i];
        }
        if (elu && v < 0.f) v = expm1f(v);   // (not <=: the device's expm1f turns -0 into +0, ELU leaves it)
    }
    y[((size_t)b * Cin * k + r) * ldy + u] = v;
}

int enc_launch_unfold(hipStream_t st, const float* x, int ldx, int Cin, const int* lens, float* y, int Lout, int k, int s, int replicate,
                      int elu, int B) {
    hipLaunchKernelGGL(enc_unfold_kernel, dim3((unsigned)((Lout + 255) / 256), Cin * k, B), dim3(256), 0, st, x, ldx, Cin, lens, y,
                       (int)enc_pitch(Lout), Lout, k, s, replicate, elu);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

// ---------------------------------------------------------------------------
// Split residual VQ encode.  z [B][2 * D][ld]: rows 0..D-1 the semantic input projection, D..2D-1 the acoustic one
// (MimiSplitResidualVectorQuantizer: both project the SAME embedding).  Stages q < n_sem continue the semantic residual,
// stage n_sem restarts from the acoustic projection.  Per stage, every entry j is scored s_j = ||e_j||^2 - 2 r.e_j
// (||e_j||^2 from load time; r.e_j an f32 fma chain over d = 0..D-1 in order: a frame's bits depend on nothing but the
// frame); the arg-min is the lowest index among equal scores (torch.argmin), and r -= e_idx.
// Workgroup = FT frames (of any clips: frame g = b * T + t), 256 threads; thread tid scores the entries
// j = p * 1024 + e * 256 + tid (e < 4) against all FT frames, reading the transposed codebook [D][CB] coalesced and the
// residuals from LDS as broadcasts.
// ---------------------------------------------------------------------------
template <int FT>
__global__ void __launch_bounds__(256) enc_rvq_kernel(const float* __restrict__ z, int ld, int T, int n_frames,
                                                      const float* __restrict__ cb, const float* __restrict__ cbt,
                                                      const float* __restrict__ n2, int nq, int CB, int D, int n_sem,
                                                      int64_t* __restrict__ codes) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* r = sm;                                   // [FT][D]
    float* red_s = sm + FT * D;                      // [4 waves][FT]
    int* red_i = (int*)(red_s + 4 * FT);             // [4 waves][FT]
    int* pick = red_i + 4 * FT;                      // [FT]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int g0 = blockIdx.x * FT;
    for (int q = 0; q < nq; q++) {
        if (q == 0 || q == n_sem) {   // (re)start the residual from the projection this half reads
            const int row0 = q == 0 ? 0 : D;
            for (int idx = tid; idx < FT * D; idx += 256) {
                const int f = idx / D, d = idx - f * D, g = g0 + f;
                float v = 0.f;
                if (g < n_frames) {
                    const int b = g / T, t = g - b * T;
                    v = z[((size_t)b * 2 * D + row0 + d) * ld + t];
                }
                r[f * D + d] = v;
            }
        }
        __syncthreads();
        const float* cbq = cbt + (size_t)q * D * CB;
        const float* n2q = n2 + (size_t)q * CB;
        float best[FT];
        int bi[FT];
#pragma unroll
        for (int f = 0; f < FT; f++) { best[f] = INFINITY; bi[f] = 0x7fffffff; }
        for (int p = 0; p < CB; p += 1024) {
            float acc[4][FT];
#pragma unroll
            for (int e = 0; e < 4; e++)
#pragma unroll
                for (int f = 0; f < FT; f++) acc[e][f] = 0.f;
            int jj[4];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int j = p + e * 256 + tid;
                jj[e] = j < CB ? j : CB - 1;   // (a clamped duplicate is never taken: its own index is checked below)
            }
            for (int d = 0; d < D; d += 4) {   // (D % 4 == 0: enc_load)
                float ev[4][4];
#pragma unroll
                for (int e = 0; e < 4; e++)
#pragma unroll
                    for (int dd = 0; dd < 4; dd++) ev[e][dd] = cbq[(size_t)(d + dd) * CB + jj[e]];
#pragma unroll
                for (int f = 0; f < FT; f++) {
                    const float4 rv = *(const float4*)(r + f * D + d);
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        acc[e][f] = fmaf(ev[e][0], rv.x, acc[e][f]);
                        acc[e][f] = fmaf(ev[e][1], rv.y, acc[e][f]);
                        acc[e][f] = fmaf(ev[e][2], rv.z, acc[e][f]);
                        acc[e][f] = fmaf(ev[e][3], rv.w, acc[e][f]);
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int j = p + e * 256 + tid;
                if (j < CB) {
                    const float nj = n2q[j];
#pragma unroll
                    for (int f = 0; f < FT; f++) {
                        const float sc = nj - 2.0f * acc[e][f];
                        if (sc < best[f]) { best[f] = sc; bi[f] = j; }   // j grows within a thread: ties keep the lower
                    }
                }
            }
        }
        // arg-min over the workgroup: (score, index) lexicographic -- a total order, so the reduction order is irrelevant
#pragma unroll
        for (int f = 0; f < FT; f++) {
            float s_ = best[f];
            int i_ = bi[f];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float os = __shfl_xor(s_, o, 64);
                const int oi = __shfl_xor(i_, o, 64);
                if (os < s_ || (os == s_ && oi < i_)) { s_ = os; i_ = oi; }
            }
            if (lane == 0) { red_s[wv * FT + f] = s_; red_i[wv * FT + f] = i_; }
        }
        __syncthreads();
        if (tid < FT) {
            float s_ = red_s[tid];
            int i_ = red_i[tid];
            for (int w2 = 1; w2 < 4; w2++) {
                const float os = red_s[w2 * FT + tid];
                const int oi = red_i[w2 * FT + tid];
                if (os < s_ || (os == s_ && oi < i_)) { s_ = os; i_ = oi; }
            }
            if (i_ < 0 || i_ >= CB) i_ = 0;   // (every score NaN: cannot happen for finite inputs; keep the gather in bounds)
            pick[tid] = i_;
            const int g = g0 + tid;
            if (g < n_frames) codes[(size_t)g * nq + q] = i_;
        }
        __syncthreads();
        const float* cbr = cb + (size_t)q * CB * D;
        for (int idx = tid; idx < FT * D; idx += 256) {
            const int f = idx / D, d = idx - f * D;
            r[f * D + d] = r[f * D + d] - cbr[(size_t)pick[f] * D + d];
        }
        __syncthreads();
    }
}

int enc_launch_rvq(hipStream_t s, const float* z, int ld, int T, int n_frames, const EncOp& op, int64_t* codes) {
    const int nf = n_frames;
    const int ft = enc_rvq_tile(nf);
    const size_t lds = ((size_t)ft * op.dim + 4 * ft) * 4 + (size_t)5 * ft * 4;
    // (at most 66 112 B, 16 frames of the loader's largest dim 1024, of the CU's 160 KiB: the runtime launches it as it is,
    // tests/test_gpu_enc_rvq.py runs that shape)
    if (ft == 16)
        hipLaunchKernelGGL(enc_rvq_kernel<16>, dim3((unsigned)((nf + 15) / 16)), dim3(256), lds, s, z, ld, T, nf, op.cbk, op.cbt, op.n2,
                           op.nq, op.cb, op.dim, op.n_sem, codes);
    else
        hipLaunchKernelGGL(enc_rvq_kernel<4>, dim3((unsigned)((nf + 3) / 4)), dim3(256), lds, s, z, ld, T, nf, op.cbk, op.cbt, op.n2,
                           op.nq, op.cb, op.dim, op.n_sem, codes);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

static float* enc_up(DeviceAllocs& mem, const float* h, size_t n) {
    float* d = nullptr;
    if (!mem.alloc(&d, n * 4) || hipMemcpy(d, h, n * 4, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return d;
}
static float* enc_up(Enc* e, const float* h, size_t n) { return enc_up(e->mem, h, n); }

bool enc_rvq_tables(DeviceAllocs& mem, const float* cbk, EncOp& op) {
    const size_t ne = (size_t)op.nq * op.cb * op.dim;
    std::vector<float> t(ne), n2((size_t)op.nq * op.cb);
    for (int q = 0; q < op.nq; q++)
        for (int j = 0; j < op.cb; j++) {
            double s = 0.0;
            for (int d = 0; d < op.dim; d++) {
                const float v = cbk[((size_t)q * op.cb + j) * op.dim + d];
                t[((size_t)q * op.dim + d) * op.cb + j] = v;
                s += (double)v * v;
            }
            n2[(size_t)q * op.cb + j] = (float)s;
        }
    op.cbk = enc_up(mem, cbk, ne);
    op.cbt = enc_up(mem, t.data(), ne);
    op.n2 = enc_up(mem, n2.data(), n2.size());
    return op.cbk && op.cbt && op.n2;
}

static void enc_destroy(Enc* e) {
    if (!e) return;
    if (e->s) hipStreamSynchronize(e->s);
    enc_pcm_release(e);
    e->mem.release();
    if (e->e0) hipEventDestroy(e->e0);
    if (e->e1) hipEventDestroy(e->e1);
    if (e->s) hipStreamDestroy(e->s);
    delete e;
}

// Runs ops [0, n_ops) on the clips already in e->pcm (lens = their sample counts).  -> the buffer holding the last
// activation, its channels and (longest) length.
int enc_run(Enc* e, int B, const std::vector<int>& lens0, int n_ops, float** out, int* outC, long* outL) {
    std::vector<int> lens(lens0);
    std::vector<int> tab((size_t)e->ops.size() * e->max_batch, 0);
    long L = *std::max_element(lens.begin(), lens.begin() + B);
    // per-op input lengths (host), uploaded once
    {
        std::vector<int> l2(lens);
        for (size_t i = 0; i < e->ops.size(); i++) {
            for (int b = 0; b < B; b++) {
                tab[i * e->max_batch + b] = l2[b];
                l2[b] = (int)enc_cols_out(e->ops[i], l2[b]);
            }
        }
        Q3_HIP(hipMemcpyAsync(e->d_lens, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, e->s), -1);
    }
    float* P[2] = {e->buf[0], e->buf[1]};   // ping-pong pair
    float* res = e->buf[2];                 // the residual a later RES_ADD reads
    float* src = e->pcm;                    // the current activation
    auto other = [&](const float* x) { return P[0] == x ? P[1] : P[0]; };   // a ping-pong buffer that is not x
    long ld = enc_pitch(L);
    const size_t nrun = n_ops < 0 ? e->ops.size() : std::min((size_t)n_ops, e->ops.size());
    for (size_t i = 0; i < nrun; i++) {
        const EncOp& op = e->ops[i];
        if (op.flags & EF_RES_SAVE) {   // the input is needed again by a later RES_ADD: its buffer becomes the residual one
            if (src != P[0] && src != P[1]) return -1;
            std::swap(P[src == P[0] ? 0 : 1], res);
        }
        float* dst = (op.flags & EF_TO_RES) ? res : other(src);
        if (op.op == EOP_CONV_IN) {
            if (enc_launch_conv_in(e->s, src, (int)ld, op, dst, (int)ld, (int)L, B, nullptr, 0, nullptr)) return -1;
        } else if (op.op == EOP_CONV || op.op == EOP_CONV_S) {
            const bool strided = op.op == EOP_CONV_S;
            const long Lo = enc_cols_out(op, L);
            if (strided) {
                if (enc_launch_unfold(e->s, src, (int)ld, op.cin, e->d_lens + i * e->max_batch, e->buf[3], (int)Lo, op.k, op.p0,
                                      (op.flags & EF_REPLICATE) ? 1 : 0, (op.flags & EF_ELU) ? 1 : 0, B))
                    return -1;
            }
            ConvArgs a = enc_conv_args(op, Lo, strided);
            a.x = strided ? e->buf[3] : src;
            a.y = dst;
            if (op.flags & EF_RES_ADD) a.res = res;
            if (voc_launch_conv(e->s, a, B, e->cfg)) return -1;
            L = Lo;
            ld = enc_pitch(L);
        } else if (op.op == EOP_NORM) {
            if (voc_launch_norm(e->s, src, op.w, op.bias, dst, op.cin, (int)L, (int)ld, 1, op.eps, B)) return -1;
        } else if (op.op == EOP_ATTN) {
            if (voc_launch_attn(e->s, src, dst, op.heads, op.head_dim, (int)L, (int)ld, op.window, op.theta, B)) return -1;
        } else if (op.op == EOP_RVQ) {
            if (enc_launch_rvq(e->s, src, (int)ld, (int)L, B * (int)L, op, e->d_codes)) return -1;
            *out = nullptr;
            *outC = op.nq;
            *outL = L;
            return 0;
        }
        if (!(op.flags & EF_TO_RES)) src = dst;   // (a conv shortcut: the activation stays)
    }
    *out = src;
    *outC = nrun ? e->ops[nrun - 1].c_act : 1;
    *outL = L;
    return 0;
}

int enc_collect_codes(Enc* e, int B, const std::vector<int>& lens, long T, int64_t* codes_out, int max_frames, int32_t* n_frames) {
    std::vector<int64_t> hc((size_t)B * T * e->nq);
    Q3_HIP(hipMemcpyAsync(hc.data(), e->d_codes, hc.size() * sizeof(int64_t), hipMemcpyDeviceToHost, e->s), -1);
    Q3_HIP(hipEventRecord(e->e1, e->s), -1);
    Q3_HIP(hipStreamSynchronize(e->s), -1);
    hipEventElapsedTime(&e->last_ms, e->e0, e->e1);
    for (int b = 0; b < B; b++) {
        const int f = (int)enc_cols_after(e->ops, e->ops.size(), lens[b]);
        n_frames[b] = f;
        int64_t* dst = codes_out + (size_t)b * max_frames * e->nq;
        std::copy(hc.begin() + (size_t)b * T * e->nq, hc.begin() + ((size_t)b * T + f) * e->nq, dst);
        std::fill(dst + (size_t)f * e->nq, dst + (size_t)max_frames * e->nq, (int64_t)-1);
    }
    return 0;
}

}  // namespace q3

using namespace q3;

extern "C" {

void enc_free(void* h) {
    enc_enter((Enc*)h);
    enc_destroy((Enc*)h);
}

void* enc_load(const char* weights, int max_batch, int max_samples) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        Q3_LOG("no HIP device available -- this library has no CPU path");
        return nullptr;
    }
    if (!weights || max_batch <= 0 || max_samples <= 0) {
        Q3_LOG("enc_load: needs a weight file, max_batch > 0 and max_samples > 0");
        return nullptr;
    }
    Pack p;
    if (!p.open(weights)) return nullptr;
    const PackTensor* prog = p.find("enc.program");
    if (!prog || prog->dtype != I32 || prog->ndim != 2 || prog->shape[1] != 8 || prog->shape[0] < 2) {
        Q3_LOG("%s holds no encoder program (tensor enc.program int32 [n][8])", weights);
        return nullptr;
    }
    Enc* e = new Enc();
    hipGetDevice(&e->device);
    e->max_batch = max_batch;
    e->max_samples = max_samples;
    e->sample_rate = (int)p.get("enc_sample_rate", 24000);
    bool ok = hipStreamCreateWithFlags(&e->s, hipStreamNonBlocking) == hipSuccess && hipEventCreate(&e->e0) == hipSuccess &&
              hipEventCreate(&e->e1) == hipSuccess;
    const int32_t* pr = (const int32_t*)prog->data;
    const int n_ops = (int)prog->shape[0];
    int C = 1;
    long L = max_samples;
    size_t max_elems = (size_t)enc_pitch(L);
    bool res_live = false, done = false;
    for (int i = 0; i < n_ops && ok; i++) {
        const int32_t* r = pr + i * 8;
        EncOp op;
        op.op = r[0];
        const std::string base = "enc.op" + std::to_string(i) + ".";
        auto vec = [&](const char* n, uint64_t ne, bool required) -> const float* {
            const PackTensor* t = p.find(base + n);
            if (!t) {
                if (required) {
                    Q3_LOG("encoder op %d needs tensor %s%s", i, base.c_str(), n);
                    ok = false;
                }
                return nullptr;
            }
            if (t->dtype != F32 || t->numel() != ne) {
                Q3_LOG("encoder op %d: tensor %s is not f32 with %llu elements", i, n, (unsigned long long)ne);
                ok = false;
                return nullptr;
            }
            return (const float*)t->data;
        };
        auto fail = [&](const char* why) {
            Q3_LOG("encoder op %d (opcode %d): %s", i, op.op, why);
            ok = false;
        };
        if (done) {
            fail("ops after the quantiser");
            break;
        }
        op.cin = r[1];
        op.cout = r[2];
        op.flags = r[5];
        if (op.op == EOP_CONV_IN) {
            op.k = r[3];
            if (i != 0 || op.cin != 1 || op.cout <= 0 || op.k < 1 || op.k > ENC_IN_MAXK || op.flags) {
                fail("the one-channel input conv must come first, 1..16 taps");
                break;
            }
            const float* w = vec("weight", (uint64_t)op.cout * op.k, true);
            const float* b = vec("bias", (uint64_t)op.cout, false);
            if (!ok) break;
            op.w = enc_up(e, w, (size_t)op.cout * op.k);
            op.bias = b ? enc_up(e, b, op.cout) : nullptr;
            ok = op.w && (!b || op.bias);
            C = op.cout;
        } else if (op.op == EOP_CONV || op.op == EOP_CONV_S) {
            op.k = r[3];
            op.p0 = r[4];
            const bool strided = op.op == EOP_CONV_S;
            const int cin_eff = strided ? op.cin * op.k : op.cin;
            const int K = strided ? 1 : op.k;
            if (op.cin != C || op.cout <= 0 || op.k < 1 || op.p0 < 1 || cin_eff % 8) {
                fail("channels do not chain, or a conv input is not a multiple of 8 channels");
                break;
            }
            if (strided ? (op.k < op.p0 || (op.flags & ~(EF_ELU | EF_REPLICATE))) :
                          ((op.flags & EF_REPLICATE) || (op.k != 1 && op.k != 3 && op.k != 7 && op.k != 2) || op.p0 > 9 ||
                           ((op.flags & EF_ELU) && ((op.k != 1 && op.k != 3) || op.cin % 16)) || ((op.flags & EF_ELU) && (op.flags & EF_GELU)))) {
                fail("conv shape / flags not built (1, 2, 3 or 7 taps, dilation <= 9; ELU input: 1 or 3 taps over 16k channels)");
                break;
            }
            if ((op.flags & EF_RES_ADD) && !res_live) {
                fail("adds a residual nothing saved");
                break;
            }
            if ((op.flags & EF_TO_RES) && (op.cout != op.cin || (op.flags & (EF_RES_SAVE | EF_RES_ADD)))) {
                fail("a shortcut conv keeps the width and neither saves nor adds a residual");
                break;
            }
            const float* w = vec("weight", (uint64_t)op.cout * op.cin * op.k, true);
            const float* b = vec("bias", (uint64_t)op.cout, false);
            if (!ok) break;
            // torch [cout][cin][k] -> [tap][row][cin'] (strided: cin' = ci * k + j, one tap) -> [cin'/8][tap][cin'%8][Mp]
            const int Mp = (op.cout + 3) / 4 * 4;
            std::vector<float> wp((size_t)(cin_eff / 8) * K * 8 * Mp, 0.f);
            for (int co = 0; co < op.cout; co++)
                for (int ci = 0; ci < op.cin; ci++)
                    for (int k = 0; k < op.k; k++) {
                        const float wv = w[((size_t)co * op.cin + ci) * op.k + k];
                        const int c2 = strided ? ci * op.k + k : ci, tap = strided ? 0 : k;
                        wp[((((size_t)(c2 >> 3) * K + tap) * 8 + (c2 & 7)) * Mp) + co] = wv;
                    }
            op.w = enc_up(e, wp.data(), wp.size());
            op.bias = b ? enc_up(e, b, op.cout) : nullptr;
            ok = op.w && (!b || op.bias);
            if (strided) {
                L = enc_cols_out(op, L);
                max_elems = std::max(max_elems, (size_t)cin_eff * enc_pitch(L));
                e->hop *= op.p0;
            }
            if (op.flags & EF_RES_SAVE) res_live = true;
            if (op.flags & EF_RES_ADD) res_live = false;
            if (op.flags & EF_TO_RES) res_live = true;
            if (!(op.flags & EF_TO_RES)) C = op.cout;
        } else if (op.op == EOP_NORM) {
            if (op.cin != C || op.cout != C || r[3] != 1 || (op.flags & ~EF_RES_SAVE)) {
                fail("a LayerNorm over the activation's channels");
                break;
            }
            op.eps = (float)((double)r[4] * 1e-9);
            const float* w = vec("weight", (uint64_t)C, true);
            const float* b = vec("bias", (uint64_t)C, true);
            if (!ok) break;
            op.w = enc_up(e, w, C);
            op.bias = enc_up(e, b, C);
            ok = op.w && op.bias;
            if (op.flags & EF_RES_SAVE) res_live = true;
        } else if (op.op == EOP_ATTN) {
            op.heads = r[3];
            op.head_dim = r[4];
            op.window = r[6];
            op.theta = (float)r[7];
            if (op.cin != C || op.heads <= 0 || op.head_dim <= 0 || op.head_dim > 128 || (op.head_dim & 1) || op.window <= 0 ||
                op.cin != 3 * op.heads * op.head_dim || op.cout != op.heads * op.head_dim) {
                fail("attention geometry ([q | k | v] head-major, even head_dim <= 128)");
                break;
            }
            C = op.cout;
        } else if (op.op == EOP_RVQ) {
            op.nq = r[2];
            op.cb = r[3];
            op.dim = r[4];
            op.n_sem = r[6];
            if (op.cin != C || op.cin != 2 * op.dim || !enc_rvq_geometry(op.nq, op.cb, op.dim, op.n_sem)) {
                fail("quantiser geometry (input = semantic | acoustic projections, dim % 4 == 0, 1 <= n_sem <= nq <= 32)");
                break;
            }
            const size_t ne = (size_t)op.nq * op.cb * op.dim;
            const float* cbk = vec("codebook", ne, true);
            if (!ok) break;
            for (size_t x = 0; x < ne && ok; x++)
                if (!std::isfinite(cbk[x])) fail("non-finite codebook entry");
            if (!ok) break;
            ok = enc_rvq_tables(e->mem, cbk, op);
            e->nq = op.nq;
            done = true;
        } else {
            fail("unknown opcode");
            break;
        }
        max_elems = std::max(max_elems, (size_t)std::max(op.cin, op.cout) * enc_pitch(L));
        op.c_act = C;
        e->ops.push_back(op);
    }
    if (ok && !done) {
        Q3_LOG("encoder program does not end with the quantiser");
        ok = false;
    }
    if (ok && ((size_t)max_batch * max_elems >= ((size_t)1 << 31))) {
        Q3_LOG("enc_load: %d clips of %d samples need activations of %zu floats, beyond the kernels' 32-bit indexing",
               max_batch, max_samples, (size_t)max_batch * max_elems);
        ok = false;
    }
    if (ok) {
        e->buf_elems = (size_t)max_batch * max_elems;
        for (int i = 0; i < 4 && ok; i++) ok = e->mem.alloc_zeroed(&e->buf[i], e->buf_elems * 4, e->s);   // (zeroed once: padding columns start finite)
        e->codes_cap = (size_t)max_batch * (size_t)((max_samples + e->hop - 1) / e->hop) * e->nq;
        ok = ok && e->mem.alloc(&e->pcm, (size_t)max_batch * enc_pitch(max_samples) * 4) &&
             e->mem.alloc(&e->d_lens, e->ops.size() * max_batch * sizeof(int)) && e->mem.alloc(&e->d_codes, e->codes_cap * sizeof(int64_t)) &&
             hipDeviceSynchronize() == hipSuccess;
    }
    if (!ok) {
        Q3_LOG("enc_load failed");
        enc_destroy(e);
        return nullptr;
    }
    return e;
}

int enc_num_quantizers(void* h) { return h ? ((Enc*)h)->nq : 0; }
int enc_sample_rate(void* h) { return h ? ((Enc*)h)->sample_rate : 0; }
int enc_samples_per_frame(void* h) { return h ? ((Enc*)h)->hop : 0; }
float enc_last_ms(void* h) { return h ? ((Enc*)h)->last_ms : -1.f; }

int enc_frames(void* h, int n) {
    Enc* e = (Enc*)h;
    if (!e || n <= 0) return -1;
    return (int)enc_cols_after(e->ops, e->ops.size(), n);   // nested ceilings compose: ceil(ceil(n / a) / b) = ceil(n / (a b))
}

// checks the arguments and uploads the clips (each row zero after its own length) -> 0 / <0
static int enc_upload(Enc* e, const float* pcm, const int32_t* n, int B, std::vector<int>& lens, const char* who) {
    if (!pcm || !n) {
        Q3_LOG("%s: NULL pcm or n_samples", who);
        return -1;
    }
    if (B < 1 || B > e->max_batch) {
        Q3_LOG("%s: B = %d outside 1..%d (max_batch)", who, B, e->max_batch);
        return -1;
    }
    lens.assign(e->max_batch, 0);
    size_t total = 0;
    for (int b = 0; b < B; b++) {
        if (n[b] <= 0 || n[b] > e->max_samples) {
            Q3_LOG("%s: clip %d has %d samples (1..%d)", who, b, n[b], e->max_samples);
            return -1;
        }
        lens[b] = n[b];
        total += (size_t)n[b];
    }
    for (size_t i = 0; i < total; i++)
        if (!std::isfinite(pcm[i])) {
            Q3_LOG("%s: sample %zu is not finite", who, i);
            return -1;
        }
    const long L = *std::max_element(lens.begin(), lens.begin() + B), ld = enc_pitch(L);
    Q3_HIP(hipMemsetAsync(e->pcm, 0, (size_t)B * ld * 4, e->s), -1);
    size_t off = 0;
    for (int b = 0; b < B; b++) {
        Q3_HIP(hipMemcpyAsync(e->pcm + (size_t)b * ld, pcm + off, (size_t)n[b] * 4, hipMemcpyHostToDevice, e->s), -1);
        off += (size_t)n[b];
    }
    return 0;
}

int enc_encode(void* h, const float* pcm, const int32_t* n_samples, int B, int64_t* codes_out, int max_frames, int32_t* n_frames) {
    Enc* e = (Enc*)h;
    if (!e) {
        Q3_LOG("enc_encode: NULL handle");
        return -1;
    }
    enc_enter(e);
    if (!codes_out || !n_frames) {
        Q3_LOG("enc_encode: NULL codes_out or n_frames");
        return -1;
    }
    if (pcm && n_samples && B >= 1 && B <= e->max_batch) {
        for (int b = 0; b < B; b++) {
            const int f = n_samples[b] > 0 ? enc_frames(e, n_samples[b]) : 0;
            if (f > max_frames) {
                Q3_LOG("enc_encode: clip %d gives %d frames, codes_out holds %d per clip", b, f, max_frames);
                return -1;
            }
        }
    }
    std::vector<int> lens;
    Q3_HIP(hipEventRecord(e->e0, e->s), -1);
    if (enc_upload(e, pcm, n_samples, B, lens, "enc_encode")) return -1;
    float* out = nullptr;
    int C = 0;
    long T = 0;
    if (enc_run(e, B, lens, -1, &out, &C, &T)) return -1;
    return enc_collect_codes(e, B, lens, T, codes_out, max_frames, n_frames);
}

// test hook (not in the header, like voc_debug_run): run the first n_ops ops on the clips and return the activation
// dense [B][C][L] (L = the longest clip's columns at that stage; out must hold B * C * L floats for the call's lengths,
// enc_debug_shape tells them).  n_ops past the last conv / norm / attention: the quantiser has no activation, -1.
int enc_debug_shape(void* h, const int32_t* n_samples, int B, int n_ops, int* C, int* L) {
    Enc* e = (Enc*)h;
    if (!e || !n_samples || B < 1 || B > e->max_batch || n_ops < 1 || n_ops >= (int)e->ops.size()) return -1;
    long Lc = 0;
    for (int b = 0; b < B; b++) Lc = std::max(Lc, (long)n_samples[b]);
    *C = e->ops[n_ops - 1].c_act;
    *L = (int)enc_cols_after(e->ops, n_ops, Lc);
    return 0;
}

int enc_debug_run(void* h, const float* pcm, const int32_t* n_samples, int B, int n_ops, float* out, int* C, int* L) {
    Enc* e = (Enc*)h;
    if (!e || !out || n_ops < 1 || n_ops >= (int)e->ops.size()) return -1;
    enc_enter(e);
    std::vector<int> lens;
    if (enc_upload(e, pcm, n_samples, B, lens, "enc_debug_run")) return -1;
    float* act = nullptr;
    long LL = 0;
    if (enc_run(e, B, lens, n_ops, &act, C, &LL) || !act) return -1;
    *L = (int)LL;
    Q3_HIP(hipMemcpy2DAsync(out, sizeof(float) * (size_t)LL, act, sizeof(float) * (size_t)enc_pitch(LL), sizeof(float) * (size_t)LL,
                            (size_t)B * (*C), hipMemcpyDeviceToHost, e->s), -1);
    Q3_HIP(hipStreamSynchronize(e->s), -1);
    return 0;
}

}  // extern "C"
