// q3_enc_stream.hip -- carry-state streaming encode (enc_stream_*, include/qwen3tts_enc_stream.h): the op table of q3_enc.hip
// run a push at a time.  Every op with a receptive field keeps, per stream, the columns its next output still reads
// ([max_streams][state_floats] on the device, zero after a reset = the causal padding); a push lays [carried | new] out in a
// work buffer, runs the op's ordinary kernel over it and drops the carried columns' outputs.
//
// Shared with the incremental vocoder (q3_voc_ops.h): the [history | new] assembly (voc_launch_incr_prepend), the attention
// over a carried k|v window with absolute positions (voc_launch_incr_attn), and -- as in enc_run, through the same op -> launch
// layer (q3_enc.h) -- the exact-fp32 MFMA conv under enc_conv_args' pin, the first conv reading its k - 1 carried samples
// (enc_launch_conv_in), the channel norm and enc_launch_rvq.  Own kernels:
//   enc_stream_unfold_kernel    strided conv input from [carry | new] -> [Cin * k][whole strides], rolling the left context and
//                               the unconsumed tail back into the carry; the clip-end padding only in the finish push
//   enc_stream_emit_kernel      columns of a group's activation -> rows of the push's packed [frame][channel] buffer
// An activation is buf[cur] = [B][C][pitch(skip + n)]: `skip` leading columns are outputs of carried columns (nothing reads
// them), n are the new ones.  No rule looks at n, skip or B, so a column's bits are those of any other split.
// A push's samples are the host's float32 (enc_stream_push), or an EncStreamFeed writes them into d_pcm's rows on the device
// (enc_stream_push_pcm, q3_enc_stream_pcm.hip); plan, walk and hand-out are the same for both.
#include "../../include/qwen3tts_enc.h"
#include "q3_enc.h"

#include <algorithm>
#include <cmath>

namespace q3 {

constexpr int ENC_S_MAXCARRY = 32;    // columns a strided op carries (k - 1)
constexpr int ENC_MAX_HIST = 256;     // columns voc_incr_prepend_kernel holds

// Strided conv input with carry (MimiConv1d: k taps, stride s, k - s columns of left context).  The stream's carry row of
// channel ci holds cnt = (k - s) + before % s columns: the left context of the next output and the columns no whole stride
// has consumed (`before` = columns this op had taken when the push started).  V = [carry | n_in new columns of x from column
// skip]; output u < n_out reads V[u * s + t], t < k:  y[b][ci * k + t][u] = act(V[u * s + t]).  The last cnt' = (k - s) +
// (before + n_in) % s columns of V become the carry.  A stream's first column (before == 0) stands in for the left padding
// where the op replicates; an index past the end of V exists only in the finish push (n_out rounds up there): zero, or the
// last column.  One workgroup per (channel, entry) owns the carry row: it is staged in LDS before anything is written.
__global__ void __launch_bounds__(256) enc_stream_unfold_kernel(const float* __restrict__ x, int ldx, int skip, int Cin, int n_in,
                                                                float* __restrict__ y, int ldy, int n_out, int k, int s, int replicate,
                                                                int elu, int finish, float* hist, long long state_floats,
                                                                const int* __restrict__ streams, const int* __restrict__ before) {
    __shared__ float cs[ENC_S_MAXCARRY];
    const int ci = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int T0 = before[b], cnt = (k - s) + T0 % s, total = cnt + n_in;
    float* h = hist + (size_t)streams[b] * state_floats + (size_t)ci * (k - 1);
    const float* xr = x + ((size_t)b * Cin + ci) * ldx + skip;
    if (tid < cnt) cs[tid] = (T0 == 0 && replicate && n_in > 0) ? xr[0] : h[tid];
    __syncthreads();
    auto V = [&](int v) -> float {
        if (v < cnt) return cs[v];
        if (v < total) return xr[v - cnt];
        if (!replicate || total == 0) return 0.f;
        return total - 1 < cnt ? cs[total - 1] : xr[total - 1 - cnt];
    };
    float* yb = y + ((size_t)b * Cin + ci) * k * ldy;
    for (int t = 0; t < k; t++)
        for (int u = tid; u < n_out; u += 256) {
            float v = V(u * s + t);
            if (elu && v < 0.f) v = expm1f(v);   // (as enc_unfold_kernel: -0 stays -0)
            yb[(size_t)t * ldy + u] = v;
        }
    if (!finish) {
        const int cnt2 = (k - s) + (T0 + n_in) % s;   // = total - n_out * s
        if (tid < cnt2) h[tid] = V(n_out * s + tid);
    }
}

// columns [skip, skip + n) of y [B][C][ld] -> out[(off[b] + j)][C]: the push's frames, entry after entry
__global__ void __launch_bounds__(256) enc_stream_emit_kernel(const float* __restrict__ y, int C, int ld, int skip, int n,
                                                              const int* __restrict__ off, float* __restrict__ out) {
    const int c = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y, b = blockIdx.z;
    if (c < C) out[((size_t)off[b] + j) * C + c] = y[((size_t)b * C + c) * ld + skip + j];
}

int enc_stream_launch_unfold(hipStream_t st, const float* x, int ldx, int skip, int Cin, int n_in, float* y, int n_out, int k, int s,
                             int replicate, int elu, int finish, float* hist, long long state_floats, const int* streams, const int* before,
                             int B) {
    hipLaunchKernelGGL(enc_stream_unfold_kernel, dim3(Cin, B), dim3(256), 0, st, x, ldx, skip, Cin, n_in, y, (int)enc_pitch(n_out), n_out, k, s,
                       replicate, elu, finish, hist, state_floats, streams, before);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}
int enc_stream_launch_emit(hipStream_t st, const float* y, int C, int ld, int skip, int n, const int* off, float* out, int B) {
    hipLaunchKernelGGL(enc_stream_emit_kernel, dim3((unsigned)((C + 255) / 256), (unsigned)n, B), dim3(256), 0, st, y, C, ld, skip, n, off, out);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

namespace {

struct Plan {
    std::vector<long long> n_frames;   // per entry
    PushGroups groups;                 // keys: n_in[0 .. n_levels], then the finish flag
};

int make_plan(const EncStream* s, int n, const int32_t* streams, const int32_t* n_new, const int32_t* finish, int source, Plan& p) {
    if (n < 0 || (n > 0 && (!streams || !n_new))) {
        Q3_LOG("enc_stream_push: NULL streams or n_new");
        return -1;
    }
    const int nl = (int)s->lev_s.size();
    p.n_frames.assign(n, 0);
    p.groups = PushGroups();
    std::vector<char> seen(s->max_streams, 0);
    std::vector<long long> key(nl + 2), bc(nl + 1), carry(nl);
    for (int i = 0; i < n; i++) {
        const int k = streams[i];
        if (k < 0 || k >= s->max_streams || seen[k] || n_new[i] < 0 || n_new[i] > s->max_push) {
            Q3_LOG("enc_stream_push: entry %d: bad stream %d (or named twice) or %d new samples (0..%d)", i, k, n_new[i], s->max_push);
            return -1;
        }
        seen[k] = 1;
        if (s->finished[k]) {
            Q3_LOG("enc_stream_push: stream %d has finished (enc_stream_reset starts the next clip)", k);
            return -1;
        }
        if (s->source[k] != ENC_SRC_NONE && s->source[k] != source) {
            Q3_LOG("enc_stream_push: stream %d: enc_stream_push and enc_stream_push_pcm do not mix on one clip (enc_stream_reset starts the next)", k);
            return -1;
        }
        if (s->total[k] + n_new[i] > 0x7fffffffLL) {
            Q3_LOG("enc_stream_push: stream %d is beyond 2^31 samples", k);
            return -1;
        }
        const bool fin = finish && finish[i];
        enc_stream_plan(s->lev_k.data(), s->lev_s.data(), nl, s->total[k], n_new[i], fin, key.data(), bc.data(), carry.data());
        key[nl + 1] = fin;
        p.n_frames[i] = key[nl];
        if (std::any_of(key.begin(), key.begin() + nl + 1, [](long long v) { return v > 0; })) p.groups.add(key, i, s->e->max_batch);
    }
    return 0;
}

// One launch sequence: B entries with the same key through the op table.  dry: no launch; -1 when an activation would not
// fit the work buffers (checked for every group of a push before its first launch).
int walk(EncStream* s, const std::vector<long long>& key, int B, bool dry, bool want_emb, int* launches) {
    Enc* e = s->e;
    const size_t nops = e->ops.size();
    const int nl = (int)s->lev_s.size(), mb = e->max_batch;
    const bool fin = key[nl + 1] != 0;
    const int* d_streams = s->d_meta;
    const int* d_foff = s->d_meta + (1 + nops) * mb;
    int cur = -1, res = -1, lvl = 0, skip = 0, res_ld = 0, res_skip = 0;
    long long n = key[0];
    auto pick = [&](int x = -1) {
        for (int j = 0; j < 4; j++)
            if (j != cur && j != res && j != x) return j;
        return -1;
    };
    auto fits = [&](int ch, long long cols) { return (size_t)B * ch * enc_pitch(cols) <= s->buf_elems; };
    auto before = [&](size_t i) { return s->d_meta + (1 + i) * mb; };
    // columns [skip, skip + n) of channels [c0, c0 + Cc) of buf[cur] behind the op's H carried columns -> dst; the history moves on
    auto prepend = [&](size_t i, int Cc, int c0, int srcC, float* dst) -> int {
        (*launches)++;
        return dry ? 0 : voc_launch_incr_prepend(e->s, s->buf[cur], srcC, c0, (int)enc_pitch(skip + n), skip, dst, Cc,
                                                 (int)enc_pitch(s->H[i] + n), s->d_hist + s->hoff[i], nullptr, nullptr, s->H[i], (int)n,
                                                 (long long)s->state_floats, d_streams, B);
    };
    auto emit = [&](int C, float* out) -> int {
        (*launches)++;
        return dry ? 0 : enc_stream_launch_emit(e->s, s->buf[cur], C, (int)enc_pitch(skip + n), skip, (int)n, d_foff, out, B);
    };
    for (size_t i = 0; i < nops; i++) {
        const EncOp& op = e->ops[i];
        const int C = i ? e->ops[i - 1].c_act : 1;   // channels of the activation the op reads
        if ((int)i == s->emb_op && want_emb && n > 0 && emit(C, s->d_emb)) return -1;
        if (op.op == EOP_CONV_S) {
            const long long n_out = key[lvl + 1];
            if (n > 0 || n_out > 0) {
                const int u = pick();
                if (!fits(op.cin * op.k, n_out)) return -1;
                (*launches)++;
                if (!dry && enc_stream_launch_unfold(e->s, cur >= 0 ? s->buf[cur] : s->buf[0], (int)enc_pitch(skip + n), skip, op.cin, (int)n,
                                                     s->buf[u], (int)n_out, op.k, op.p0, (op.flags & EF_REPLICATE) ? 1 : 0,
                                                     (op.flags & EF_ELU) ? 1 : 0, fin ? 1 : 0, s->d_hist + s->hoff[i],
                                                     (long long)s->state_floats, d_streams, before(i), B))
                    return -1;
                if (n_out > 0) {
                    const int d = pick(u);
                    if (d < 0 || !fits(op.cout, n_out)) return -1;
                    ConvArgs a = enc_conv_args(op, n_out, true);
                    a.x = s->buf[u];
                    a.y = s->buf[d];
                    (*launches)++;
                    if (!dry && voc_launch_conv(e->s, a, B, e->cfg)) return -1;
                    cur = d;
                }
            }
            n = n_out;
            skip = 0;
            lvl++;
            continue;
        }
        if (n == 0) continue;   // no new column at this level: the op's history stays
        if (op.op == EOP_CONV_IN) {
            const int d = pick();
            if (!fits(op.cout, n)) return -1;
            (*launches)++;
            if (!dry && enc_launch_conv_in(e->s, s->d_pcm, (int)enc_pitch(s->max_push), op, s->buf[d], (int)enc_pitch(n), (int)n, B,
                                           s->d_hist + s->hoff[i], (long long)s->state_floats, d_streams))
                return -1;
            cur = d;
            skip = 0;
        } else if (op.op == EOP_CONV) {
            if (cur < 0) return -1;
            if (s->H[i] > 0) {   // the whole activation becomes [history | new] (pre-ELU: the conv applies it while staging)
                const int d = pick();
                if (d < 0 || !fits(C, s->H[i] + n)) return -1;
                if (prepend(i, C, 0, C, dry ? nullptr : s->buf[d])) return -1;
                cur = d;
                skip = s->H[i];
            }
            const long long cols = skip + n;
            const int ld = (int)enc_pitch(cols);
            if (op.flags & EF_RES_SAVE) res = cur, res_ld = ld, res_skip = skip;
            int tmp = -1;
            ConvArgs a = enc_conv_args(op, cols, false);
            if (op.flags & EF_RES_ADD) {
                if (res < 0) return -1;
                if (res_ld != ld || res_skip != skip) {
                    // the residual was saved at another column offset (a shortcut conv ahead of a conv that carries a history):
                    // its new columns move to where this conv's output has them
                    tmp = pick();
                    if (tmp < 0 || !fits(op.cout, cols)) return -1;
                    (*launches)++;
                    if (!dry && voc_launch_incr_prepend(e->s, s->buf[res], op.cout, 0, res_ld, res_skip, s->buf[tmp] + skip, op.cout, ld,
                                                        nullptr, nullptr, nullptr, 0, (int)n, 0, d_streams, B))
                        return -1;
                    a.res = s->buf[tmp];
                } else {
                    a.res = s->buf[res];
                }
            }
            const int d = pick(tmp);
            if (d < 0 || !fits(op.cout, cols)) return -1;
            a.x = s->buf[cur];
            a.y = s->buf[d];
            (*launches)++;
            if (!dry && voc_launch_conv(e->s, a, B, e->cfg)) return -1;
            if (op.flags & EF_RES_ADD) res = -1;
            if (op.flags & EF_TO_RES) {   // a conv shortcut: the activation stays
                res = d;
                res_ld = ld;
                res_skip = skip;
            } else {
                cur = d;
            }
        } else if (op.op == EOP_NORM) {
            if (cur < 0) return -1;
            const long long cols = skip + n;
            if (op.flags & EF_RES_SAVE) res = cur, res_ld = (int)enc_pitch(cols), res_skip = skip;
            const int d = pick();
            if (d < 0 || !fits(op.cin, cols)) return -1;
            (*launches)++;
            if (!dry && voc_launch_norm(e->s, s->buf[cur], op.w, op.bias, s->buf[d], op.cin, (int)cols, (int)enc_pitch(cols), 1, op.eps, B))
                return -1;
            cur = d;
        } else if (op.op == EOP_ATTN) {
            // k | v rows of the new columns join the carried window in d_kv; q stays where it is and the output keeps the input's
            // columns, so the residual saved before the q/k/v projection lines up with it
            if (cur < 0) return -1;
            const int HD = op.heads * op.head_dim, Hk = s->H[i];
            if ((size_t)B * 2 * HD * enc_pitch(Hk + n) > s->kv_elems) return -1;
            if (prepend(i, 2 * HD, HD, 3 * HD, dry ? nullptr : s->d_kv)) return -1;
            const int d = pick();
            if (d < 0 || !fits(HD, skip + n)) return -1;
            (*launches)++;
            if (!dry && voc_launch_incr_attn(e->s, s->buf[cur], (int)enc_pitch(skip + n), skip, s->d_kv, (int)enc_pitch(Hk + n), Hk, s->buf[d],
                                             op.heads, op.head_dim, op.window, op.theta, before(i), (int)n, B))
                return -1;
            cur = d;
        } else if (op.op == EOP_RVQ) {
            if (cur < 0 || C != 2 * op.dim) return -1;
            if (emit(C, s->d_z)) return -1;   // the quantiser runs once over the frames of the whole push
        }
    }
    return 0;
}

}  // namespace

int enc_stream_push_impl(EncStream* s, int n, const int32_t* streams, const float* pcm, const int32_t* n_new, const int32_t* finish,
                         int64_t* codes_out, int64_t cap, int64_t* offsets, float* emb_out, int* emb_channels, EncStreamFeed* feed) {
    if (!s || !offsets) {
        Q3_LOG("enc_stream_push: NULL object or offsets");
        return -1;
    }
    Enc* e = s->e;
    enc_enter(e);
    Plan p;
    const int source = feed ? ENC_SRC_PCM : ENC_SRC_F32;
    if (make_plan(s, n, streams, n_new, finish, source, p)) return -1;
    long long frames = 0;
    size_t samples = 0;
    std::vector<size_t> poff(n, 0);
    for (int i = 0; i < n; i++) {
        poff[i] = samples;
        samples += (size_t)n_new[i];
        frames += p.n_frames[i];
    }
    if (frames > cap || (frames > 0 && !codes_out) || (samples > 0 && !pcm && !feed) || (size_t)frames > s->frames_cap) {
        Q3_LOG("enc_stream_push: %lld frames do not fit the caller's buffer of %lld (or no samples given)", frames, (long long)cap);
        return -1;
    }
    for (size_t i = 0; !feed && i < samples; i++)
        if (!std::isfinite(pcm[i])) {
            Q3_LOG("enc_stream_push: sample %zu is not finite", i);
            return -1;
        }
    int dry_launches = 0;
    for (size_t g = 0; g < p.groups.keys.size(); g++)
        if (walk(s, p.groups.keys[g], (int)p.groups.members[g].size(), true, emb_out != nullptr, &dry_launches)) {
            Q3_LOG("enc_stream_push: a push does not fit the object's work buffers");
            return -1;
        }
    if (feed && feed->begin() < 0) return -1;
    // the push is valid
    long long at = 0;
    for (int i = 0; i < n; i++) offsets[i] = at, at += p.n_frames[i];
    offsets[n] = at;
    if (emb_channels) *emb_channels = s->emb_C;
    const size_t nops = e->ops.size();
    const int nl = (int)s->lev_s.size(), mb = e->max_batch;
    const long ldp = enc_pitch(s->max_push);
    std::vector<std::vector<int>> metas(p.groups.keys.size());   // (alive until the stream has drained: the uploads are asynchronous)
    std::vector<long long> key(nl + 2), bc(nl + 1), carry(nl);
    s->last_launches = 0;
    s->last_ms = 0.f;
    if (!p.groups.keys.empty()) Q3_HIP(hipEventRecord(e->e0, e->s), -1);
    for (size_t g = 0; g < p.groups.keys.size(); g++) {
        const std::vector<int>& mem = p.groups.members[g];
        const int B = (int)mem.size();
        std::vector<int>& meta = metas[g];
        meta.assign((2 + nops) * mb, 0);
        for (int b = 0; b < B; b++) {
            const int en = mem[b], k = streams[en];
            enc_stream_plan(s->lev_k.data(), s->lev_s.data(), nl, s->total[k], n_new[en], finish && finish[en], key.data(), bc.data(),
                            carry.data());
            meta[b] = k;
            for (size_t i = 0; i < nops; i++) meta[(1 + i) * mb + b] = (int)bc[s->level_of[i]];
            meta[(1 + nops) * mb + b] = (int)offsets[en];
            if (n_new[en] > 0 && !feed)
                Q3_HIP(hipMemcpyAsync(s->d_pcm + (size_t)b * ldp, pcm + poff[en], sizeof(float) * (size_t)n_new[en], hipMemcpyHostToDevice, e->s), -1);
        }
        Q3_HIP(hipMemcpyAsync(s->d_meta, meta.data(), sizeof(int) * meta.size(), hipMemcpyHostToDevice, e->s), -1);
        if (feed && p.groups.keys[g][0] > 0) {
            const int r = feed->fill(mem, p.groups.keys[g][0]);
            if (r < 0) return -1;
            s->last_launches += r;
        }
        if (walk(s, p.groups.keys[g], B, false, emb_out != nullptr, &s->last_launches)) return -1;
    }
    if (feed) {
        const int r = feed->end();
        if (r < 0) return -1;
        s->last_launches += r;
    }
    if (frames > 0) {
        const EncOp& q = e->ops.back();
        if (enc_launch_rvq(e->s, s->d_z, 1, 1, (int)frames, q, s->d_codes)) return -1;   // frame g: 2 * dim floats at g * 2 * dim
        s->last_launches++;
        Q3_HIP(hipMemcpyAsync(codes_out, s->d_codes, sizeof(int64_t) * (size_t)frames * e->nq, hipMemcpyDeviceToHost, e->s), -1);
        if (emb_out)
            Q3_HIP(hipMemcpyAsync(emb_out, s->d_emb, sizeof(float) * (size_t)frames * s->emb_C, hipMemcpyDeviceToHost, e->s), -1);
    }
    if (!p.groups.keys.empty()) Q3_HIP(hipEventRecord(e->e1, e->s), -1);
    Q3_HIP(hipStreamSynchronize(e->s), -1);
    if (!p.groups.keys.empty()) hipEventElapsedTime(&s->last_ms, e->e0, e->e1);
    for (int i = 0; i < n; i++) {
        s->total[streams[i]] += n_new[i];
        s->source[streams[i]] = (char)source;
        if (finish && finish[i]) s->finished[streams[i]] = 1;
    }
    return 0;
}

int enc_stream_plan_frames(const EncStream* s, int n, const int32_t* streams, const int32_t* n_new, const int32_t* finish, int source) {
    Plan p;
    if (!s || make_plan(s, n, streams, n_new, finish, source, p)) return -1;
    long long t = 0;
    for (int i = 0; i < n; i++) t += p.n_frames[i];
    return (int)t;
}

}  // namespace q3

using namespace q3;

extern "C" {

void enc_stream_free(void* ss) {
    EncStream* s = (EncStream*)ss;
    if (!s) return;
    enc_enter(s->e);
    hipStreamSynchronize(s->e->s);
    enc_stream_pcm_release(s);
    delete s;   // (its allocations go with it: DeviceAllocs)
}

void* enc_stream_create(void* h, int max_streams, int max_push_samples) {
    Enc* e = (Enc*)h;
    if (!e || max_streams <= 0 || max_push_samples <= 0) {
        Q3_LOG("enc_stream_create: needs an encoder handle, max_streams > 0 and max_push_samples > 0");
        return nullptr;
    }
    enc_enter(e);
    EncStream* s = new EncStream;
    s->e = e;
    s->max_streams = max_streams;
    s->max_push = max_push_samples;
    s->total.assign(max_streams, 0);
    s->finished.assign(max_streams, 0);
    s->source.assign(max_streams, ENC_SRC_NONE);
    const size_t nops = e->ops.size();
    s->H.assign(nops, 0);
    s->hoff.assign(nops, 0);
    s->level_of.assign(nops, 0);
    auto refuse = [&](size_t i, const char* why) -> void* {
        Q3_LOG("enc_stream_create: op %zu (opcode %d) cannot be streamed: %s", i, e->ops[i].op, why);
        delete s;
        return nullptr;
    };
    // per op: what it carries.  Work buffers: level l sees at most ceil(max_push / P_l) + 1 new columns in a push (P_l: the
    // product of the strides above it; + 1: the column the finish push pads out) behind at most ENC_MAX_HIST carried ones.
    size_t need = 0, need_kv = 0;
    long long P = 1;
    auto nmax = [&]() { return (long long)(max_push_samples + P - 1) / P + 1; };
    for (size_t i = 0; i < nops; i++) {
        const EncOp& op = e->ops[i];
        s->level_of[i] = (int)s->lev_s.size();
        int chans = 0;
        switch (op.op) {
            case EOP_CONV_IN:
                if (i != 0) return refuse(i, "the input conv is not the first op");
                s->H[i] = op.k - 1;
                chans = 1;
                break;
            case EOP_CONV:
                s->H[i] = (op.k - 1) * op.p0;
                chans = op.cin;
                break;
            case EOP_CONV_S:
                if (op.k - 1 > ENC_S_MAXCARRY || op.k < op.p0) return refuse(i, "a strided conv carries at most 32 columns");
                s->H[i] = op.k - 1;
                chans = op.cin;
                break;
            case EOP_ATTN:
                s->H[i] = op.window - 1;
                chans = 2 * op.heads * op.head_dim;
                break;
            case EOP_NORM:
            case EOP_RVQ: break;
            default: return refuse(i, "no carried form of this op is built");
        }
        if (op.op != EOP_CONV_S && s->H[i] > ENC_MAX_HIST) return refuse(i, "it carries more than the 256 columns the history kernel holds");
        s->hoff[i] = s->state_floats;
        s->state_floats += (size_t)s->H[i] * chans;
        const long long cols = nmax() + ENC_MAX_HIST;
        if (op.op == EOP_ATTN) need_kv = std::max(need_kv, (size_t)chans * enc_pitch(s->H[i] + nmax()));
        if (op.op == EOP_RVQ) break;
        need = std::max(need, (size_t)std::max(i ? e->ops[i - 1].c_act : 1, std::max(op.cin, op.cout)) * enc_pitch(cols));
        if (op.op == EOP_CONV_S) {
            s->lev_k.push_back(op.k);
            s->lev_s.push_back(op.p0);
            P *= op.p0;
            need = std::max(need, (size_t)op.cin * op.k * enc_pitch(nmax()));
        }
    }
    // the embedding is the input of the projection in front of the quantiser
    if (nops < 3 || e->ops[nops - 1].op != EOP_RVQ || e->ops[nops - 2].op != EOP_CONV || e->ops[nops - 2].k != 1)
        return refuse(nops - 1, "the quantiser does not follow a one-tap projection");
    s->emb_op = (int)nops - 2;
    s->emb_C = e->ops[nops - 2].cin;
    const size_t mb = (size_t)e->max_batch;
    if (mb * need >= ((size_t)1 << 31) || mb * need_kv >= ((size_t)1 << 31)) {
        Q3_LOG("enc_stream_create: %d entries of %d samples need activations beyond the kernels' 32-bit indexing", e->max_batch, max_push_samples);
        delete s;
        return nullptr;
    }
    s->buf_elems = need * mb;
    s->kv_elems = std::max<size_t>(1, need_kv * mb);
    s->frames_cap = (size_t)max_streams * ((size_t)max_push_samples / e->hop + 2);
    const EncOp& q = e->ops.back();
    DeviceAllocs& m = s->mem;
    const size_t slack = 1024;   // (float4 groups past a row's last column)
    bool ok = m.alloc_zeroed(&s->d_hist, sizeof(float) * std::max<size_t>(1, s->state_floats * max_streams), e->s);
    for (int i = 0; i < 4; i++) ok = ok && m.alloc_zeroed(&s->buf[i], sizeof(float) * (s->buf_elems + slack), e->s);   // (zeroed once: dropped columns start finite)
    ok = ok && m.alloc_zeroed(&s->d_kv, sizeof(float) * (s->kv_elems + slack), e->s) &&
         m.alloc_zeroed(&s->d_pcm, sizeof(float) * mb * enc_pitch(max_push_samples), e->s) &&
         m.alloc_zeroed(&s->d_meta, sizeof(int) * (2 + nops) * mb, e->s) && m.alloc(&s->d_z, sizeof(float) * s->frames_cap * 2 * q.dim) &&
         m.alloc(&s->d_emb, sizeof(float) * s->frames_cap * s->emb_C) && m.alloc(&s->d_codes, sizeof(int64_t) * s->frames_cap * q.nq) &&
         hipStreamSynchronize(e->s) == hipSuccess;
    if (!ok) {
        Q3_LOG("enc_stream_create: device allocation failed");
        delete s;
        return nullptr;
    }
    return s;
}

int enc_stream_reset(void* ss, int stream) {
    EncStream* s = (EncStream*)ss;
    if (!s || stream < 0 || stream >= s->max_streams) return -1;
    enc_enter(s->e);
    if (s->state_floats)   // the causal padding again (ordered before the next push on the handle's stream)
        Q3_HIP(hipMemsetAsync(s->d_hist + (size_t)stream * s->state_floats, 0, sizeof(float) * s->state_floats, s->e->s), -1);
    s->total[stream] = 0;
    s->finished[stream] = 0;
    s->source[stream] = ENC_SRC_NONE;
    return 0;
}

int enc_stream_push_max_frames(void* s, int n, const int32_t* streams, const int32_t* n_new, const int32_t* finish) {
    return enc_stream_plan_frames((EncStream*)s, n, streams, n_new, finish, ENC_SRC_F32);
}

int enc_stream_push(void* s, int n, const int32_t* streams, const float* pcm, const int32_t* n_new, const int32_t* finish,
                    int64_t* codes_out, int64_t out_capacity_frames, int64_t* offsets) {
    return enc_stream_push_impl((EncStream*)s, n, streams, pcm, n_new, finish, codes_out, out_capacity_frames, offsets, nullptr, nullptr);
}

float enc_stream_last_ms(void* s) { return s ? ((EncStream*)s)->last_ms : -1.f; }
int enc_stream_last_launches(void* s) { return s ? ((EncStream*)s)->last_launches : -1; }
int64_t enc_stream_state_bytes(void* s) { return s ? (int64_t)(((EncStream*)s)->state_floats * sizeof(float)) : -1; }
int64_t enc_stream_device_bytes(void* s) { return s ? (int64_t)((EncStream*)s)->mem.bytes : -1; }

}  // extern "C"
