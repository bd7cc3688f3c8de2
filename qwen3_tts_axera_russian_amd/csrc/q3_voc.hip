// q3_voc.hip -- fp32 vocoder (codec ids -> waveform) for gfx950, include/qwen3tts_voc.h.
//
// Stands where the reference calls onnxruntime on the traced Qwen3TTSTokenizerV2 decoder
// (dual_npu/vocoder_server.py:67-71; scripts/export_vocoder_traced.py:38-52).  The decoder's layer
// list is not in the reference, so the library interprets an op table from the weight container
// (tensor `voc.program`, int32 [n_ops][8]); DESIGN.md documents the table and the default one
// (split-RVQ de-quantiser -> causal conv -> x2 x2 transposed-conv upsamplers -> BigVGAN-style
// decoder: rates 8,5,4,3, residual units with dilations 1,3,9, Snake activations).
//
// This file: the loader, the op -> launch layer and the chunk decode (voc_run, voc_decode).  The kernels and their launchers are
// q3_voc_kernels.hip (q3_voc_ops.h); the chunk walk, voc_stream_* and voc_incr_* are q3_voc_stream.hip (q3_voc_program.h).
#include "../../include/qwen3tts_voc.h"
#include "q3_voc_program.h"

#include <algorithm>
#include <cmath>
#include <utility>

namespace q3 {

// host -> device on the handle's stream, complete on return (loading: the source may be a temporary)
static bool voc_upload(Voc* v, void* d, const void* src, size_t bytes) {
    return hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, v->s) == hipSuccess && hipStreamSynchronize(v->s) == hipSuccess;
}

// device -> the caller's (pageable) memory, complete on return: DMA into the pinned staging on the handle's stream, then a
// host copy -- a pageable destination would be chunked through the runtime's own staging buffers instead
int voc_read_back(Voc* v, void* out, const void* dev, size_t bytes) {
    for (size_t o = 0; o < bytes; o += v->h_stage_bytes) {
        const size_t n = bytes - o < v->h_stage_bytes ? bytes - o : v->h_stage_bytes;
        Q3_HIP(hipMemcpyAsync(v->h_stage, (const char*)dev + o, n, hipMemcpyDeviceToHost, v->s), -1);
        Q3_HIP(hipStreamSynchronize(v->s), -1);
        memcpy((char*)out + o, v->h_stage, n);
    }
    return 0;
}

static float* voc_up(Voc* v, const PackTensor* t) {
    size_t ne = t->numel();
    std::vector<float> tmp;
    const float* src = (const float*)t->data;
    if (t->dtype == F16) {
        tmp.resize(ne);
        for (size_t i = 0; i < ne; i++) tmp[i] = h2f(((const uint16_t*)t->data)[i]);
        src = tmp.data();
    } else if (t->dtype != F32) {
        return nullptr;
    }
    float* d = nullptr;
    if (hipMalloc((void**)&d, ne * 4) != hipSuccess) return nullptr;
    v->allocs.push_back(d);
    if (!voc_upload(v, d, src, ne * 4)) return nullptr;
    return d;
}

static float* voc_up_host(Voc* v, const std::vector<float>& h) {
    float* d = nullptr;
    if (hipMalloc((void**)&d, h.size() * 4) != hipSuccess) return nullptr;
    v->allocs.push_back(d);
    if (!voc_upload(v, d, h.data(), h.size() * 4)) return nullptr;
    return d;
}

static void voc_destroy(Voc* v) {
    if (!v) return;
    if (v->s) hipStreamSynchronize(v->s);
    for (void* p : v->allocs) hipFree(p);
    for (float* b : v->buf)
        if (b) hipFree(b);
    for (_Float16* b : v->plane)
        if (b) hipFree(b);
    if (v->d_codes) hipFree(v->d_codes);
    if (v->d_wave) hipFree(v->d_wave);
    if (v->d_wave16) hipFree(v->d_wave16);
    if (v->d_place) hipFree(v->d_place);
    if (v->d_ovf) hipFree(v->d_ovf);
    if (v->d_snap) hipFree(v->d_snap);
    if (v->d_snap_tab) hipFree(v->d_snap_tab);
    if (v->h_stage) hipHostFree(v->h_stage);
    if (v->h_ovf) hipHostFree(v->h_ovf);
    if (v->e0) hipEventDestroy(v->e0);
    if (v->e1) hipEventDestroy(v->e1);
    if (v->s) hipStreamDestroy(v->s);
    delete v;
}

}  // namespace q3

using namespace q3;

extern "C" {

void voc_free(void* vv) {
    voc_enter((Voc*)vv);
    voc_destroy((Voc*)vv);
}

void* voc_load(const char* weights, int chunk_tokens, int max_batch) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        Q3_LOG("no HIP device available -- this library has no CPU path");
        return nullptr;
    }
    if (!weights) return nullptr;
    Pack p;
    if (!p.open(weights)) return nullptr;
    const PackTensor* prog = p.find("voc.program");
    if (!prog || prog->dtype != I32 || prog->ndim != 2 || prog->shape[1] != 8) {
        Q3_LOG("%s holds no vocoder program (tensor voc.program int32 [n][8])", weights);
        return nullptr;
    }
    // (any chunk length decodes; the chunk walk needs chunk > 32 and says so itself: plan_walk)
    if (const char* ex = getenv("Q3_VOC_EXACT")) voc_settings.set_exact_fp32(atoi(ex));
    Voc* v = new Voc();
    hipGetDevice(&v->device);
    v->chunk = chunk_tokens > 0 ? chunk_tokens : 64;
    v->max_batch = max_batch > 0 ? max_batch : 1;
    bool ok = true;
    {
        // lowest queue priority: the vocoder is throughput work that runs beside the latency-bound frame
        // loop (highest priority, q3_engine.hip); Q3_STREAM_PRIO=0 creates both at the default priority, =2 this one only
        int lo = 0, hi = 0;
        const int mode = getenv("Q3_STREAM_PRIO") ? atoi(getenv("Q3_STREAM_PRIO")) : 1;
        const bool prio = mode != 0 && mode != 2;
        if (prio && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && lo != hi)
            ok = hipStreamCreateWithPriority(&v->s, hipStreamNonBlocking, lo) == hipSuccess;
        else
            ok = hipStreamCreateWithFlags(&v->s, hipStreamNonBlocking) == hipSuccess;
    }
    ok = ok && hipEventCreate(&v->e0) == hipSuccess && hipEventCreate(&v->e1) == hipSuccess;
    const int32_t* pr = (const int32_t*)prog->data;
    const int n_ops = (int)prog->shape[0];
    int C = 0;
    long L = v->chunk;
    size_t max_elems = 0;
    double flops = 0.0;
    for (int i = 0; i < n_ops && ok; i++) {
        const int32_t* r = pr + i * 8;
        VocOp op;
        op.op = r[0];
        const std::string base = "voc.op" + std::to_string(i) + ".";
        auto need = [&](const char* n) -> const PackTensor* {
            const PackTensor* t = p.find(base + n);
            if (!t) {
                Q3_LOG("vocoder program op %d needs tensor %s%s", i, base.c_str(), n);
                ok = false;
            }
            return t;
        };
        if (op.op == VOP_EMBMEAN) {
            op.nq = r[1];
            op.cb = r[2];
            op.cout = r[3];  // embedding width
            const PackTensor* tb = need("embedding");
            if (!ok) break;
            if (op.nq < 1 || op.nq > 16 || tb->numel() != (uint64_t)op.nq * op.cb * op.cout) {
                Q3_LOG("vocoder op %d: embedding table size does not match the program (1..16 quantisers)", i);
                ok = false;
                break;
            }
            op.w = voc_up(v, tb);
            ok = op.w != nullptr;
            C = op.cout;
        } else if (op.op == VOP_RVQ) {
            op.nq = r[1];
            op.cb = r[2];
            op.cin = r[3];   // codebook dim
            op.cout = r[4];  // output channels
            const PackTensor *cb = need("codebook"), *ps = need("proj_sem"), *pa = need("proj_ac");
            if (!ok) break;
            if (op.nq < 1 || op.nq > 16) {
                Q3_LOG("vocoder op %d: %d quantisers (a request carries 16 ids per frame)", i, op.nq);
                ok = false;
                break;
            }
            if (cb->numel() != (uint64_t)op.nq * op.cb * op.cin || ps->numel() != (uint64_t)op.cout * op.cin ||
                pa->numel() != (uint64_t)op.cout * op.cin) {
                Q3_LOG("vocoder op %d: RVQ tensor sizes do not match the program", i);
                ok = false;
                break;
            }
            op.w = voc_up(v, cb);
            op.p_sem = voc_up(v, ps);
            op.p_ac = voc_up(v, pa);
            ok = op.w && op.p_sem && op.p_ac;
            C = op.cout;
            flops += 2.0 * 2 * op.cin * op.cout * L;
        } else if (op.op == VOP_CONV || op.op == VOP_CONVT) {
            op.cin = r[1];
            op.cout = r[2];
            op.k = r[3];
            op.p0 = r[4];  // dilation (conv) or stride (convT)
            op.flags = r[5];
            if (op.op == VOP_CONVT) {
                op.lt = r[6];
                op.rt = r[7];
                // every kept output must come from the polyphase GEMM over the input's own columns (+ k/s - 1 more)
                if (op.lt < 0 || op.rt < 0 || op.p0 <= 0 || op.lt + op.rt > op.k || convt_out(op, L) <= 0) {
                    Q3_LOG("vocoder op %d: transposed conv k=%d s=%d cannot be trimmed by %d + %d", i, op.k, op.p0, op.lt, op.rt);
                    ok = false;
                    break;
                }
            }
            if (op.cin != C) {
                Q3_LOG("vocoder op %d: expects %d input channels, previous op produced %d", i, op.cin, C);
                ok = false;
                break;
            }
            const PackTensor *wt = need("weight"), *bs = p.find(base + "bias");
            if (!ok) break;
            if (wt->numel() != (uint64_t)op.cin * op.cout * op.k || wt->dtype != F32) {
                Q3_LOG("vocoder op %d: weight size/dtype does not match the program", i);
                ok = false;
                break;
            }
            // repack to [tap][row][cin]
            const float* src = (const float*)wt->data;
            std::vector<float> wk;
            if (op.op == VOP_CONV) {  // torch Conv1d weight [cout][cin][k]
                wk.resize((size_t)op.k * op.cout * op.cin);
                for (int co = 0; co < op.cout; co++)
                    for (int ci = 0; ci < op.cin; ci++)
                        for (int k = 0; k < op.k; k++)
                            wk[((size_t)k * op.cout + co) * op.cin + ci] = src[((size_t)co * op.cin + ci) * op.k + k];
            } else {  // torch ConvTranspose1d weight [cin][cout][k], k = J*stride: polyphase rows m = co*s + p,
                      // tap j (input offset -j) reads w[ci][co][p + j*s]; conv tap index kk = J-1-j.  Row m of input
                      // column l is output sample l*s + p of the untrimmed result; op.lt / op.rt samples are cut
                      // at the ends (both k - s in the decoder family's CausalTransConvNet; 0 / k - s = strictly causal).
                const int s = op.p0;
                const int J = s > 0 ? op.k / s : 0;
                if (s <= 0 || J < 1 || op.k != J * s) {
                    Q3_LOG("vocoder op %d: transposed conv needs kernel = J*stride (got k=%d s=%d)", i, op.k, s);
                    ok = false;
                    break;
                }
                wk.resize((size_t)J * op.cout * s * op.cin);
                for (int j = 0; j < J; j++)
                    for (int co = 0; co < op.cout; co++)
                        for (int ph = 0; ph < s; ph++)
                            for (int ci = 0; ci < op.cin; ci++)
                                wk[((size_t)(J - 1 - j) * op.cout * s + (size_t)co * s + ph) * op.cin + ci] =
                                    src[((size_t)ci * op.cout + co) * op.k + ph + j * s];
            }
            if (op.cin % 16 == 0) {   // split-precision copy: [cin/16][tap][Mp128][16] hi / lo fp16
                const int KTAPS = op.op == VOP_CONV ? op.k : op.k / op.p0;
                const int Mrows = op.op == VOP_CONV ? op.cout : op.cout * op.p0;
                const int Mp = Mrows % 96 == 0 ? Mrows : (Mrows + 127) / 128 * 128;   // 96- or 64-row tiles, in bounds
                std::vector<uint16_t> hi((size_t)(op.cin / 16) * KTAPS * Mp * 16, 0), lo(hi.size(), 0);
                bool in_range = true;   // a weight beyond the fp16 range keeps this op on the exact path
                for (int k = 0; k < KTAPS; k++)
                    for (int m = 0; m < Mrows; m++)
                        for (int ci = 0; ci < op.cin; ci++) {
                            const float wv = wk[((size_t)k * Mrows + m) * op.cin + ci];
                            in_range = in_range && fabsf(wv) <= 65504.f;
                            const uint16_t h = f2h_sat(wv);
                            const size_t d = ((((size_t)(ci >> 4) * KTAPS + k) * Mp) + m) * 16 + (ci & 15);
                            hi[d] = h;
                            lo[d] = f2h_sat((wv - h2f(h)) * 2048.0f);
                        }
                void *dh = nullptr, *dl = nullptr;
                if (in_range) {
                    if (hipMalloc(&dh, hi.size() * 2) != hipSuccess || hipMalloc(&dl, lo.size() * 2) != hipSuccess) {
                        ok = false;
                        break;
                    }
                    v->allocs.push_back(dh);
                    v->allocs.push_back(dl);
                    ok = voc_upload(v, dh, hi.data(), hi.size() * 2) && voc_upload(v, dl, lo.data(), lo.size() * 2);
                    op.w_hi = (_Float16*)dh;
                    op.w_lo = (_Float16*)dl;
                    op.Mp128 = Mp;
                    if (!ok) break;
                }
            }
            if (op.op == VOP_CONV && op.k == 1 && op.cin == op.cout && resunit_channels(op.cin) &&
                (op.flags & VF_RES_ADD) && (op.flags & VF_SNAKE)) {
                // resunit_kernel's order: w1p[row tile][t = (mt, q)][lane = (h, m)] = W[32 tile + m][32 mt + (q&3) + 8 (q>>2) + 4 h]
                const int Cc = op.cin;
                std::vector<float> w1((size_t)Cc * Cc);
                for (int t2 = 0; t2 < Cc / 32; t2++)
                    for (int t = 0; t < Cc / 2; t++)
                        for (int ln = 0; ln < 64; ln++) {
                            const int mt = t / 16, q = t % 16, h = ln >> 5, m = ln & 31;
                            const int c = 32 * mt + (q & 3) + 8 * (q >> 2) + 4 * h;
                            w1[((size_t)t2 * (Cc / 2) + t) * 64 + ln] = wk[(size_t)(32 * t2 + m) * Cc + c];
                        }
                op.w1p = voc_up_host(v, w1);
                if (!op.w1p) {
                    ok = false;
                    break;
                }
            }
            {   // [tap][row][cin] -> stage-major [cin/8][tap][cin%8][Mp]
                const int KTAPS = op.op == VOP_CONV ? op.k : op.k / op.p0;
                const int Mrows = op.op == VOP_CONV ? op.cout : op.cout * op.p0;
                const int Mp = (Mrows + 3) / 4 * 4;
                std::vector<float> wp((size_t)(op.cin / 8) * KTAPS * 8 * Mp, 0.f);
                for (int k = 0; k < KTAPS; k++)
                    for (int m = 0; m < Mrows; m++)
                        for (int ci = 0; ci < op.cin; ci++)
                            wp[((((size_t)(ci >> 3) * KTAPS + k) * 8 + (ci & 7)) * Mp) + m] =
                                wk[((size_t)k * Mrows + m) * op.cin + ci];
                wk.swap(wp);
            }
            op.w = voc_up_host(v, wk);
            op.bias = bs ? voc_up(v, bs) : nullptr;
            if (op.flags & VF_SNAKE) {
                const PackTensor *al = need("alpha"), *be = need("beta");
                if (!ok) break;
                // SnakeBeta with log-scale parameters: x + sin^2(exp(a) x) / (exp(b) + 1e-9)
                std::vector<float> ha(op.cin), hb(op.cin);
                for (int c = 0; c < op.cin; c++) {
                    const float av = al->dtype == F32 ? ((const float*)al->data)[c] : h2f(((const uint16_t*)al->data)[c]);
                    const float bv = be->dtype == F32 ? ((const float*)be->data)[c] : h2f(((const uint16_t*)be->data)[c]);
                    ha[c] = expf(av);
                    hb[c] = 1.0f / (expf(bv) + 1e-9f);
                }
                op.alpha = voc_up_host(v, ha);
                op.inv_beta = voc_up_host(v, hb);
            }
            if (op.cin % 8) {
                Q3_LOG("vocoder op %d: Cin=%d is not a multiple of 8", i, op.cin);
                ok = false;
                break;
            }
            ok = ok && op.w;
            flops += 2.0 * op.cin * op.cout * op.k * L;  // per input column; convT: k taps spread over s outputs
            C = op.cout;
            if (op.op == VOP_CONVT) L = convt_out(op, L);
        } else if (op.op == VOP_DWCONV || op.op == VOP_NORM || op.op == VOP_ATTN || op.op == VOP_GLU) {
            op.cin = r[1];
            op.cout = r[2];
            op.flags = r[5];
            if (op.cin != C) {
                Q3_LOG("vocoder op %d: expects %d input channels, previous op produced %d", i, op.cin, C);
                ok = false;
                break;
            }
            auto vec = [&](const char* n, uint64_t ne, bool required) -> float* {
                const PackTensor* t = p.find(base + n);
                if (!t) {
                    if (required) {
                        Q3_LOG("vocoder program op %d needs tensor %s%s", i, base.c_str(), n);
                        ok = false;
                    }
                    return nullptr;
                }
                if (t->numel() != ne) {
                    Q3_LOG("vocoder op %d: tensor %s has %llu elements, the program needs %llu", i, n,
                           (unsigned long long)t->numel(), (unsigned long long)ne);
                    ok = false;
                    return nullptr;
                }
                float* d = voc_up(v, t);
                if (!d) ok = false;
                return d;
            };
            if (op.op == VOP_DWCONV) {          // torch depthwise Conv1d weight [C][1][k]
                op.k = r[3];
                if (op.cout != op.cin || op.k < 1 || op.k > 64) ok = false;
                op.w = vec("weight", (uint64_t)op.cin * op.k, true);
                op.bias = vec("bias", (uint64_t)op.cin, false);
                flops += 2.0 * op.cin * op.k * L;
            } else if (op.op == VOP_NORM) {
                op.kind = r[3];
                op.eps = (float)((double)r[4] * 1e-9);
                if (op.cout != op.cin || (op.kind != 0 && op.kind != 1)) ok = false;
                op.w = vec("weight", (uint64_t)op.cin, true);
                op.bias = vec("bias", (uint64_t)op.cin, false);
            } else if (op.op == VOP_ATTN) {
                op.heads = r[3];
                op.head_dim = r[4];
                op.window = r[6];
                op.theta = (float)r[7];
                if (op.heads <= 0 || op.head_dim <= 0 || op.head_dim > 128 || (op.head_dim & 1) || op.window <= 0 ||
                    op.cin != 3 * op.heads * op.head_dim || op.cout != op.heads * op.head_dim)
                    ok = false;
                flops += 4.0 * op.heads * op.head_dim * (double)(op.window < L ? op.window : L) * L;
            } else {
                op.kind = r[3];   // 0 SiLU, 1 GELU
                if (op.cin != 2 * op.cout || (op.kind != 0 && op.kind != 1)) ok = false;
            }
            if (!ok) {
                Q3_LOG("vocoder op %d: malformed program row / tensors", i);
                break;
            }
            C = op.cout;
            if ((size_t)op.cin * pitch4(L) > max_elems) max_elems = (size_t)op.cin * pitch4(L);
        } else {
            Q3_LOG("vocoder program op %d: unknown opcode %d", i, op.op);
            ok = false;
            break;
        }
        if ((size_t)C * pitch4(L) > max_elems) max_elems = (size_t)C * pitch4(L);
        v->ops.push_back(op);
    }
    if (ok && C != 1) {
        Q3_LOG("vocoder program must end with 1 channel (got %d)", C);
        ok = false;
    }
    if (ok) {
        // nominal samples per frame = the product of the strides (decoder.total_upsample,
        // scripts/export_vocoder_traced.py:46: what the callers' SAMPLES_PER_TOKEN is); a decode returns chunk_samples
        long up = 1;
        for (const VocOp& o : v->ops)
            if (o.op == VOP_CONVT) up *= o.p0;
        v->upsample = (int)up;
        v->chunk_samples = L;
        if (L > (long)v->chunk * up) {
            Q3_LOG("vocoder program yields %ld samples for %d frames, more than %ld per frame", L, v->chunk, up);
            ok = false;
        }
    }
    if (ok) {
        v->flops_per_chunk = flops;
        v->buf_elems = max_elems * v->max_batch;
        for (int i = 0; i < 3 && ok; i++)     // (zeroed once: pad columns start finite)
            ok = hipMalloc((void**)&v->buf[i], v->buf_elems * 4) == hipSuccess && hipMemsetAsync(v->buf[i], 0, v->buf_elems * 4, v->s) == hipSuccess;
        for (int i = 0; i < 4 && ok; i++) ok = hipMalloc((void**)&v->plane[i], v->buf_elems * 2) == hipSuccess;
        ok = ok && hipMalloc((void**)&v->d_codes, sizeof(int64_t) * 16 * v->chunk * v->max_batch) == hipSuccess;
        ok = ok && hipMalloc((void**)&v->d_ovf, 16) == hipSuccess && hipMemsetAsync(v->d_ovf, 0, 16, v->s) == hipSuccess;
        ok = ok && hipMalloc((void**)&v->d_place, sizeof(ChunkPlace) * v->max_batch) == hipSuccess;
        // every read-back goes through this pinned block on the handle's stream: one decode of max_batch chunks fits whole
        v->h_stage_bytes = sizeof(float) * (size_t)v->chunk_samples * v->max_batch;
        if (v->h_stage_bytes < 4096) v->h_stage_bytes = 4096;
        ok = ok && hipHostMalloc((void**)&v->h_stage, v->h_stage_bytes, 0) == hipSuccess;
        ok = ok && hipHostMalloc((void**)&v->h_ovf, 16, 0) == hipSuccess;
        ok = ok && hipStreamSynchronize(v->s) == hipSuccess;   // the zeroing above
    }
    if (!ok) {
        Q3_LOG("voc_load failed");
        voc_destroy(v);
        return nullptr;
    }
    return v;
}

}  // extern "C"

// the process's settings: written here and by the setters of q3_voc_kernels.hip, loaded by entry points only (q3_voc_settings.h)
q3::VocSettingsStore q3::voc_settings;

extern "C" {

// 1: every call decodes on the exact-fp32 MFMA path; 0 (default): the split-precision fp16 path where it is built.  Process-wide,
// from the next call on (q3_voc_settings.h).
int voc_set_exact_fp32(int on) {
    voc_settings.set_exact_fp32(on);
    return 0;
}

int voc_set_fused_units(int on) {   // 1 (default): residual units at 96 / 192 channels run as one launch (exact path)
    voc_settings.set_fused_units(on);
    return 0;
}

int voc_chunk_tokens(void* vv) { return vv ? ((Voc*)vv)->chunk : 0; }
int voc_samples_per_token(void* vv) { return vv ? ((Voc*)vv)->upsample : 0; }
int voc_chunk_samples(void* vv) { return vv ? (int)((Voc*)vv)->chunk_samples : 0; }
float voc_last_decode_ms(void* vv) { return vv ? ((Voc*)vv)->last_ms : -1.f; }
double voc_decode_flops(void* vv, int B) { return vv ? ((Voc*)vv)->flops_per_chunk * B : 0.0; }

}  // extern "C"

namespace q3 {

// ---- op -> launch (q3_voc_program.h): the one place where an op of the table becomes a kernel launch.  voc_run below, the
// incremental walk (q3_voc_stream.hip) and voc_conv_split go through it, so the two decodes cannot drift apart. ----
int voc_op_embed(const Voc* v, const VocOp& op, const int64_t* codes, float* out, int T, int B) {
    const int ld = (int)pitch4(T);
    if (op.op == VOP_RVQ) return voc_launch_rvq(v->s, codes, op.w, op.p_sem, op.p_ac, out, T, ld, op.nq, op.cb, op.cin, op.cout, B);
    return voc_launch_embmean(v->s, codes, op.w, out, T, ld, op.nq, 16, op.cb, op.cout, B);
}

int voc_op_pointwise(const Voc* v, const VocOp& op, const float* in, float* out, long cols, int B) {
    const int L = (int)cols, ld = (int)pitch4(cols);
    switch (op.op) {
        case VOP_DWCONV: return voc_launch_dwconv(v->s, in, op.w, op.bias, out, op.cin, L, ld, op.k, B);
        case VOP_NORM: return voc_launch_norm(v->s, in, op.w, op.bias, out, op.cin, L, ld, op.kind, op.eps, B);
        case VOP_GLU: return voc_launch_glu(v->s, in, out, op.cout, L, ld, op.kind, B);
        default: return -1;
    }
}

// The GEMM a conv op is over `cols` input columns: a causal conv as it stands, a transposed conv as its polyphase form (k / s
// taps, cout * s virtual rows, the whole-chunk trims).  ConvArgs and SplitArgs both take their geometry from here.
struct ConvGeom {
    int K, dil, stride, M, lt, Lout, Lc;
};
static ConvGeom voc_conv_geom(const VocOp& op, long cols) {
    if (op.op == VOP_CONV) return {op.k, op.p0, 1, op.cout, 0, (int)cols, (int)cols};
    return {op.k / op.p0, 1, op.p0, op.cout * op.p0, op.lt, (int)convt_out(op, cols), (int)convt_cols(op, cols)};
}

ConvArgs voc_conv_args(const VocOp& op, long cols, long Lf) {
    const ConvGeom g = voc_conv_geom(op, cols);
    ConvArgs a;
    a.wk = op.w;
    a.bias = op.bias;
    a.alpha = op.alpha;
    a.inv_beta = op.inv_beta;
    a.Cin = op.cin;
    a.Cout = op.cout;
    a.clamp = (op.flags & VF_CLAMP) ? 1 : 0;
    a.gelu = (op.flags & VF_GELU) ? 1 : 0;
    a.K = g.K, a.dil = g.dil, a.stride = g.stride, a.M = g.M, a.lt = g.lt, a.Lout = g.Lout, a.Lc = g.Lc;
    a.Lin = (int)cols;
    a.Lrule = (int)(op.op == VOP_CONV ? Lf : convt_cols(op, Lf));
    a.ldx = (int)pitch4(cols);
    a.ldy = (int)pitch4(a.Lout);
    return a;
}

ResUnitArgs voc_resunit_args(const VocOp& op, const VocOp& op1, const float* in, float* out, long cols) {
    ResUnitArgs ra;
    ra.x = in;
    ra.y = out;
    ra.w7 = op.w;
    ra.w1p = op1.w1p;
    ra.b7 = op.bias;
    ra.b1 = op1.bias;
    ra.al7 = op.alpha;
    ra.ib7 = op.inv_beta;
    ra.al1 = op1.alpha;
    ra.ib1 = op1.inv_beta;
    ra.Lin = (int)cols;
    ra.ld = (int)pitch4(cols);
    ra.dil = op.p0;
    return ra;
}

bool voc_fused_unit(const Voc* v, size_t i, size_t n_ops) {
    const VocOp& op = v->ops[i];
    return v->cfg.fuse && op.op == VOP_CONV && op.k == 7 && (op.flags & VF_RES_SAVE) && (op.flags & VF_SNAKE) && op.cin == op.cout &&
           resunit_channels(op.cin) && i + 1 < n_ops && v->ops[i + 1].w1p;
}

bool voc_split_capable(const VocOp& op) { return (op.op == VOP_CONV || op.op == VOP_CONVT) && op.w_hi != nullptr; }

// (a GELU consumer takes its planes from the separate pass: erf in the conv's epilogue costs every conv registers)
bool voc_split_emits_planes(const VocOp& op, const VocOp* next) {
    return next && voc_split_capable(*next) && op.op == VOP_CONV && op.cout % 16 == 0 && !(next->flags & VF_GELU);
}

SplitArgs voc_split_args(const VocOp& op, long cols) {
    const ConvGeom g = voc_conv_geom(op, cols);
    SplitArgs sa;
    sa.w_hi = op.w_hi;
    sa.w_lo = op.w_lo;
    sa.bias = op.bias;
    sa.Cin = op.cin;
    sa.Cout = op.cout;
    sa.Mp = op.Mp128;
    sa.Lin = (int)cols;
    sa.clamp = (op.flags & VF_CLAMP) ? 1 : 0;
    sa.dil = g.dil, sa.stride = g.stride, sa.M = g.M, sa.lt = g.lt, sa.Lout = g.Lout, sa.Lc = g.Lc;
    sa.ldy = (int)pitch4(sa.Lout);
    return sa;
}

void voc_split_out_planes(SplitArgs& sa, const VocOp& next, _Float16* oh, _Float16* ol) {
    sa.oh = oh;
    sa.ol = ol;
    if (next.flags & VF_SNAKE) {
        sa.oalpha = next.alpha;
        sa.oinv_beta = next.inv_beta;
    }
}

int voc_split_taps(const VocOp& op) { return voc_conv_geom(op, 1).K; }

// Split path of one conv op.  State carried between ops: which f32 buffer holds the newest f32 activation
// (and whether it is the current one), and which plane set (if any) already holds the current activation in
// the next conv's input form.
struct SplitState {
    int f32_idx = 0;
    bool f32_cur = true;
    int planes = -1;       // plane set holding the current activation (Snake of the consuming op applied), or -1
    float* res = nullptr;  // residual-unit input (f32)
};


static int voc_conv_split(Voc* v, const VocOp& op, const VocOp* next, bool last, int B, long L, SplitState& st) {
    int in_set = st.planes;
    if (in_set < 0) {   // materialise the input planes from the f32 activation (this op's Snake applied)
        if (!st.f32_cur) return -1;
        in_set = 0;
        if (voc_launch_snake_split(v->s, v->buf[st.f32_idx], op.alpha, op.inv_beta, v->plane[0], v->plane[1], op.cin, (int)L, (int)pitch4(L),
                                   (op.flags & VF_GELU) ? 1 : 0, v->d_ovf, B))
            return -1;
    }
    if (op.flags & VF_RES_SAVE) {
        if (!st.f32_cur) return -1;   // the producer keeps an f32 copy whenever its consumer saves a residual
        st.res = v->buf[st.f32_idx];
    }
    const bool want_planes = voc_split_emits_planes(op, next);
    const bool want_f32 = !want_planes || last || (next->flags & VF_RES_SAVE);
    SplitArgs sa = voc_split_args(op, L);
    sa.xh = v->plane[2 * in_set];
    sa.xl = v->plane[2 * in_set + 1];
    sa.ovf = v->d_ovf;
    sa.res = (op.flags & VF_RES_ADD) ? st.res : nullptr;
    int out_f32 = st.f32_idx;
    if (want_f32) {
        // never the buffer the residual (or a still-current f32 input) lives in
        out_f32 = st.f32_idx ^ 1;
        if (sa.res == v->buf[out_f32]) return -1;
        sa.y = v->buf[out_f32];
    }
    if (want_planes) voc_split_out_planes(sa, *next, v->plane[2 * (in_set ^ 1)], v->plane[2 * (in_set ^ 1) + 1]);
    if (launch_conv_split(v->s, sa, voc_split_taps(op), B, v->cfg)) return -1;
    if (want_f32) {
        st.f32_idx = out_f32;
        st.f32_cur = true;
    } else {
        st.f32_cur = false;
    }
    st.planes = want_planes ? (in_set ^ 1) : -1;
    return 0;
}

// T: frames per chunk of THIS decode (0 = the model's chunk length).  Every op is causal per column apart from the
// transposed convs' look-ahead of one input column (< 1 frame in total), so the first n frames' samples of a decode of
// T > n frames are the same bits whatever T is: the chunk walk decodes a short tail chunk at its own length + 1 pad frame
// instead of the reference's zero-padded 64 (d_codes then holds [B][T][16]).
int voc_run(Voc* v, int B, float** out_dev, int n_ops, int* outC, long* outL, float* op_ms, bool force_exact, int T) {
    // ping-pong between buf[0]/buf[1]; buf[2] keeps the residual-unit input (exact path)
    int cur = 0, C = 0;
    if (T <= 0 || T > v->chunk) T = v->chunk;
    long L = T;
    long Lf = v->chunk;   // the same op's length in a full-length decode (variant rules look at it)
    float* res = nullptr;
    SplitState st;
    // an op has written the f32 activation buf[cur ^ 1]: it becomes the current one
    auto wrote_f32 = [&]() {
        cur ^= 1;
        st.f32_idx = cur;
        st.f32_cur = true;
        st.planes = -1;
    };
    // the unit's input is needed again two ops later: it becomes buf[2] (a pointer swap, no copy), where the ping-pong of the
    // ops in between does not write
    auto save_res = [&]() {
        std::swap(v->buf[2], v->buf[cur]);
        return res = st.res = v->buf[2];
    };
    const size_t nrun = n_ops < 0 ? v->ops.size() : (size_t)n_ops < v->ops.size() ? (size_t)n_ops : v->ops.size();
    for (size_t i = 0; i < nrun; i++) {
        const VocOp& op = v->ops[i];
        const size_t i0 = i;   // (a fused unit takes op i + 1 with it: its time is booked on i0)
        if (op_ms) hipEventRecord(v->e0, v->s);
        if (op.op == VOP_RVQ || op.op == VOP_EMBMEAN) {
            if (voc_op_embed(v, op, v->d_codes, v->buf[cur ^ 1], T, B)) return -1;
            C = op.cout;
            wrote_f32();
        } else if (op.op == VOP_DWCONV || op.op == VOP_NORM || op.op == VOP_ATTN || op.op == VOP_GLU) {
            if (!st.f32_cur) return -1;   // these ops read the f32 activation (their producer wrote one: they are no conv)
            cur = st.f32_idx;
            float* out = v->buf[cur ^ 1];
            const float* in = (op.flags & VF_RES_SAVE) ? save_res() : v->buf[cur];
            if (op.op == VOP_ATTN) {
                // the variant follows the full-length decode's Lf (a short decode runs its model's kernel: same bits per
                // column); the LDS follows this decode's L <= Lf
                const size_t tile_lds_full = (size_t)3 * Lf * (op.head_dim + 1) * sizeof(float);
                const bool tile = op.head_dim <= 64 && op.head_dim % 2 == 0 && tile_lds_full <= 64 * 1024;
                if ((tile ? voc_launch_attn_tile : voc_launch_attn)(v->s, in, out, op.heads, op.head_dim, (int)L, (int)pitch4(L), op.window,
                                                                    op.theta, B))
                    return -1;
            } else if (voc_op_pointwise(v, op, in, out, L, B)) {
                return -1;
            }
            C = op.cout;
            wrote_f32();
        } else if (v->cfg.split && !force_exact && op.w_hi) {
            const bool last = i + 1 == nrun;
            const VocOp* next = (i + 1 < v->ops.size()) ? &v->ops[i + 1] : nullptr;
            if (voc_conv_split(v, op, last ? nullptr : next, last, B, L, st)) {
                Q3_LOG("vocoder op %zu: split path could not be scheduled", i);
                return -1;
            }
            cur = st.f32_idx;
            C = op.cout;
            if (op.op == VOP_CONVT) L = convt_out(op, L), Lf = convt_out(op, Lf);
        } else if (voc_fused_unit(v, i, nrun) && st.f32_cur) {
            // a whole residual unit (this 7-tap conv + the 1x1 conv that closes it) in one launch
            cur = st.f32_idx;
            if (launch_resunit(v->s, voc_resunit_args(op, v->ops[i + 1], v->buf[cur], v->buf[cur ^ 1], L), op.cin, B, v->cfg)) return -1;
            wrote_f32();
            i++;   // the 1x1 conv is done
            if (op_ms) op_ms[i] = 0.f;
        } else {
            if (!st.f32_cur) return -1;
            cur = st.f32_idx;
            ConvArgs a = voc_conv_args(op, L, Lf);
            a.y = v->buf[cur ^ 1];
            a.x = (op.flags & VF_RES_SAVE) ? save_res() : v->buf[cur];
            if (op.flags & VF_RES_ADD) a.res = res ? res : st.res;
            if (voc_launch_conv(v->s, a, B, v->cfg)) return -1;
            C = op.cout;
            if (op.op == VOP_CONVT) L = convt_out(op, L), Lf = convt_out(op, Lf);
            wrote_f32();
        }
        if (op_ms) {
            hipEventRecord(v->e1, v->s);
            hipStreamSynchronize(v->s);
            hipEventElapsedTime(&op_ms[i0], v->e0, v->e1);
        }
    }
    if (!st.f32_cur) return -1;
    *out_dev = v->buf[st.f32_idx];
    if (outC) *outC = C;
    if (outL) *outL = L;
    return 0;
}

}  // namespace q3

extern "C" {

int voc_decode(void* vv, const int64_t* codes, int B, float* out) {
    Voc* v = (Voc*)vv;
    voc_enter(v);
    if (!v || !codes || !out || B <= 0 || B > v->max_batch) return -1;
    Q3_HIP(hipMemcpyAsync(v->d_codes, codes, sizeof(int64_t) * 16 * (size_t)v->chunk * B, hipMemcpyHostToDevice, v->s), -1);
    // rows of chunk_samples floats at the device pitch -> dense [B][chunk_samples] in the pinned staging -> out
    const size_t row = sizeof(float) * (size_t)v->chunk_samples, dpitch = sizeof(float) * (size_t)pitch4(v->chunk_samples);
    // one timed decode into the staging; the first attempt also fetches the split path's overflow flag
    auto attempt = [&](bool exact) -> int {
        float* res = nullptr;
        Q3_HIP(hipEventRecord(v->e0, v->s), -1);
        if (voc_run(v, B, &res, -1, nullptr, nullptr, nullptr, exact)) return -1;
        Q3_HIP(hipEventRecord(v->e1, v->s), -1);
        if (!exact) *v->h_ovf = 0;
        if (!exact && v->cfg.split) Q3_HIP(hipMemcpyAsync(v->h_ovf, v->d_ovf, sizeof(int), hipMemcpyDeviceToHost, v->s), -1);
        Q3_HIP(hipMemcpy2DAsync(v->h_stage, row, res, dpitch, row, (size_t)B, hipMemcpyDeviceToHost, v->s), -1);
        Q3_HIP(hipStreamSynchronize(v->s), -1);
        return 0;
    };
    if (attempt(false)) return -1;
    if (*v->h_ovf) {
        // an activation beyond +-65504 (or a NaN): two fp16 terms cannot carry it -- this call is redone on the
        // exact-fp32 MFMA path, so the split arithmetic never degrades a result silently
        if (!v->warned_ovf) Q3_LOG("vocoder: activation outside the fp16 range, decoding this call with the exact-fp32 path");
        v->warned_ovf = true;
        Q3_HIP(hipMemsetAsync(v->d_ovf, 0, sizeof(int), v->s), -1);
        if (attempt(true)) return -1;
    }
    memcpy(out, v->h_stage, row * (size_t)B);
    hipEventElapsedTime(&v->last_ms, v->e0, v->e1);
    return 0;
}

// test hook: per-op GPU milliseconds of one decode of B chunks (codes already uploaded by a previous voc_decode)
int voc_debug_profile(void* vv, int B, float* op_ms, int max_ops) {
    Voc* v = (Voc*)vv;
    voc_enter(v);
    if (!v || B <= 0 || B > v->max_batch || (int)v->ops.size() > max_ops) return -1;
    float* res = nullptr;
    if (voc_run(v, B, &res, -1, nullptr, nullptr, op_ms)) return -1;
    return (int)v->ops.size();
}

// test hook: run only the first n_ops ops, return the activation [B][C][L]
int voc_debug_run(void* vv, const int64_t* codes, int B, int n_ops, float* out, int* C, int* L) {
    Voc* v = (Voc*)vv;
    voc_enter(v);
    if (!v || B <= 0 || B > v->max_batch) return -1;
    Q3_HIP(hipMemcpyAsync(v->d_codes, codes, sizeof(int64_t) * 16 * (size_t)v->chunk * B, hipMemcpyHostToDevice, v->s), -1);
    float* res = nullptr;
    long LL = 0;
    if (voc_run(v, B, &res, n_ops, C, &LL)) return -1;
    *L = (int)LL;
    Q3_HIP(hipMemcpy2DAsync(out, sizeof(float) * (size_t)LL, res, sizeof(float) * (size_t)pitch4(LL), sizeof(float) * (size_t)LL,
                            (size_t)B * (*C), hipMemcpyDeviceToHost, v->s), -1);
    Q3_HIP(hipStreamSynchronize(v->s), -1);
    return 0;
}

}  // extern "C"
