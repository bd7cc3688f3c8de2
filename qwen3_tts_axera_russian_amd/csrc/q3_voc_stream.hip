// q3_voc_stream.hip -- the vocoder's entry points above one chunk decode (include/qwen3tts_voc.h): the reference's chunk walk
// (voc_synthesize*), the same walk fed frame by frame (voc_stream_*), and the carry-state incremental decode (voc_incr_*), which
// walks the op table itself through the op -> launch layer it shares with voc_run (q3_voc_program.h).
#include "../../include/qwen3tts_voc.h"
#include "q3_voc_program.h"

#include <algorithm>
#include <utility>

using namespace q3;

extern "C" {

// Frames a chunk of `len` real frames is decoded at: its own length plus the one pad frame the transposed convs' look-ahead
// reaches into (voc_run's note), rounded up to 8 so that a request's tail chunks fall into few groups; the full chunk for a
// full chunk, under the split-f16 arithmetic (its overflow redo is per call) and with Q3_VOC_FULL_CHUNKS=1 (A/B knob).
static int voc_decode_frames(const Voc* v, int len) {
    static const int full = getenv("Q3_VOC_FULL_CHUNKS") ? atoi(getenv("Q3_VOC_FULL_CHUNKS")) : 0;
    static const int rnd = getenv("Q3_VOC_FRAME_ROUND") ? atoi(getenv("Q3_VOC_FRAME_ROUND")) : 8;
    if (full || v->cfg.split || len >= v->chunk) return v->chunk;
    const int r = rnd > 0 ? rnd : 1;
    const int t = (len + 1 + r - 1) / r * r;
    return t < v->chunk ? t : v->chunk;
}

int voc_synthesize_max_samples(void* vv, int n) {
    Voc* v = (Voc*)vv;
    if (!v || n <= 0) return 0;
    return (n + v->chunk) * v->upsample;  // the reference's redundant tail chunk adds < chunk frames
}

// ---- VocoderServer.synthesize (vocoder_server.py:73-121), bug-compatible chunk walk, for U utterances at once ----
namespace {
struct WalkChunk { int utt, start, len; size_t cl; int head; long long dst; };

// the reference's walk for one utterance of n frames whose output starts at sample `base` -> its chunks, returns its length
// (<0: the chunk is too short for the walk)
long long plan_walk(const Voc* v, int u, int n, long long base, std::vector<WalkChunk>& out) {
    const int CH = v->chunk, SPT = v->upsample;
    const size_t CS = (size_t)v->chunk_samples, OV = (size_t)16 * SPT;
    if (n > CH && CH <= 32) {
        // the walk steps by chunk - 16 and its output bound (n + chunk) frames needs chunk > 32; the reference's models are
        // traced at 64 or 256 (scripts/export_vocoder_traced.py)
        Q3_LOG("vocoder chunk walk: chunk_tokens=%d is too short for the 16-frame overlap walk (need > 32)", CH);
        return -1;
    }
    // numpy slicing, as the reference writes it: `audio[:len * SAMPLES_PER_TOKEN]` of what the model returned -- a decode
    // yields chunk_samples <= CH * SPT samples (the decoder family's transposed convs trim) (vocoder_server.py:81,98-99)
    auto sliced = [&](int len) -> size_t { return (size_t)len * SPT < CS ? (size_t)len * SPT : CS; };
    if (n <= CH) {
        out.push_back({u, 0, n, sliced(n), 0, base});
        return (long long)sliced(n);
    }
    size_t have = 0;
    for (int start = 0; start < n; start += CH - 16) {
        const int len = (start + CH <= n) ? CH : n - start;
        const size_t cl = sliced(len);
        if (start == 0) {
            out.push_back({u, start, len, cl, 0, base});
            have = cl;
        } else if (have >= OV && cl >= OV) {
            out.push_back({u, start, len, cl, (int)OV, base + (long long)(have - OV)});
            have += cl - OV;
        } else {
            out.push_back({u, start, len, cl, 0, base + (long long)have});
            have += cl;
        }
    }
    return (long long)have;
}

extern "C++" {   // (the walk helpers sit inside the extern "C" block of the entry points)
// Decodes the chunks of a walk max_batch at a time -- one decode length per call: full chunks first, then the tail chunks by
// length (voc_decode_frames) -- and places each into `wave` at its dst (voc_place_copy/blend).  chunk_codes(c) -> the first frame
// of walk[c].  restore() runs before each attempt: a call in which an activation leaves the fp16 range on the split path has the
// whole walk redone on the exact-fp32 path (voc_decode's rule), so restore() must put back whatever the blends read of `wave`.
// -> 0 and *n_calls decodes (of the attempt that stands), GPU time between v->e0 and v->e1; <0 on error.
template <class ChunkCodes, class Restore>
int decode_walk(Voc* v, const std::vector<WalkChunk>& walk, ChunkCodes chunk_codes, float* wave, Restore restore, int* n_calls) {
    const int CH = v->chunk, OV = 16 * v->upsample;
    std::vector<int> order(walk.size()), frames(walk.size());
    for (size_t i = 0; i < walk.size(); i++) order[i] = (int)i, frames[i] = voc_decode_frames(v, walk[i].len);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return frames[x] > frames[y]; });
    std::vector<int64_t> padded((size_t)v->max_batch * CH * 16);
    std::vector<ChunkPlace> place(v->max_batch);
    bool redo_exact = false;
    for (int attempt = 0; attempt < 2; attempt++) {
        Q3_HIP(hipEventRecord(v->e0, v->s), -1);
        if (restore()) return -1;
        int calls = 0;
        for (size_t c0 = 0; c0 < walk.size();) {
            const int T = frames[order[c0]];
            int B = 0;
            while (c0 + B < walk.size() && B < v->max_batch && frames[order[c0 + B]] == T) B++;
            std::fill(padded.begin(), padded.begin() + (size_t)B * T * 16, 0);
            for (int b = 0; b < B; b++) {
                const WalkChunk& w = walk[order[c0 + b]];
                memcpy(padded.data() + (size_t)b * T * 16, chunk_codes(order[c0 + b]), sizeof(int64_t) * 16 * w.len);
                place[b] = {b, (int)w.cl, w.head, w.dst};
            }
            Q3_HIP(hipMemcpyAsync(v->d_codes, padded.data(), sizeof(int64_t) * 16 * (size_t)T * B, hipMemcpyHostToDevice, v->s), -1);
            Q3_HIP(hipMemcpyAsync(v->d_place, place.data(), sizeof(ChunkPlace) * B, hipMemcpyHostToDevice, v->s), -1);
            float* res = nullptr;
            long LL = 0;
            if (voc_run(v, B, &res, -1, nullptr, &LL, nullptr, redo_exact, T)) return -1;
            for (int b = 0; b < B; b++)
                if ((long)place[b].len > LL) {
                    Q3_LOG("vocoder chunk walk: a decode of %d frames yields %ld samples, fewer than the %d kept", T, LL, place[b].len);
                    return -1;
                }
            if (voc_launch_place(v->s, res, (int)pitch4(LL), v->d_place, wave, OV, B)) return -1;
            Q3_HIP(hipStreamSynchronize(v->s), -1);   // the staging vectors are reused by the next batch
            c0 += B;
            calls++;
        }
        Q3_HIP(hipEventRecord(v->e1, v->s), -1);
        *v->h_ovf = 0;
        if (v->cfg.split && !redo_exact) Q3_HIP(hipMemcpyAsync(v->h_ovf, v->d_ovf, sizeof(int), hipMemcpyDeviceToHost, v->s), -1);
        Q3_HIP(hipStreamSynchronize(v->s), -1);
        *n_calls = calls;
        if (!*v->h_ovf) break;
        // an activation beyond the fp16 range: the whole walk is redone on the exact-fp32 path
        if (!v->warned_ovf) Q3_LOG("vocoder: activation outside the fp16 range, decoding this request with the exact-fp32 path");
        v->warned_ovf = true;
        Q3_HIP(hipMemsetAsync(v->d_ovf, 0, sizeof(int), v->s), -1);
        redo_exact = true;
    }
    return 0;
}

// grows a device buffer to hold n elements of T (contents not kept)
template <typename T>
int grow(T** p, size_t* cap, size_t n) {
    if (n <= *cap) return 0;
    if (*p) hipFree(*p);
    *p = nullptr;
    *cap = 0;
    Q3_HIP(hipMalloc((void**)p, sizeof(T) * n), -1);
    *cap = n;
    return 0;
}

}  // extern "C++"

int synth_batch(Voc* v, const int64_t* codes, const int32_t* n_tokens, int U, int64_t* offsets, bool want16, void* out, int64_t cap) {
    voc_enter(v);
    if (!v || !codes || !n_tokens || !offsets || !out || U <= 0) return -1;
    std::vector<WalkChunk> walk;
    std::vector<size_t> code_off(U);
    long long total = 0;
    size_t coff = 0;
    for (int u = 0; u < U; u++) {
        if (n_tokens[u] <= 0) {
            Q3_LOG("voc_synthesize_batch: utterance %d has %d frames", u, n_tokens[u]);
            return -1;
        }
        const long long len = plan_walk(v, u, n_tokens[u], total, walk);
        if (len < 0) return -1;
        offsets[u] = total;
        code_off[u] = coff;
        coff += (size_t)n_tokens[u] * 16;
        total += len;
    }
    offsets[U] = total;
    if (total > cap) {
        Q3_LOG("voc_synthesize_batch: %lld samples do not fit the caller's buffer of %lld", total, (long long)cap);
        return -1;
    }
    if (grow(&v->d_wave, &v->wave_cap, (size_t)total)) return -1;
    int calls = 0;
    if (decode_walk(v, walk, [&](int c) { return codes + code_off[walk[c].utt] + (size_t)walk[c].start * 16; }, v->d_wave,
                    [] { return 0; }, &calls))
        return -1;
    hipEventElapsedTime(&v->batch_ms, v->e0, v->e1);
    v->batch_chunks = (int)walk.size();
    if (!want16) {
        if (voc_read_back(v, out, v->d_wave, sizeof(float) * (size_t)total)) return -1;
    } else {
        if (grow(&v->d_wave16, &v->wave16_cap, (size_t)total)) return -1;
        if (voc_launch_to_int16(v->s, v->d_wave, v->d_wave16, total)) return -1;
        if (voc_read_back(v, out, v->d_wave16, sizeof(int16_t) * (size_t)total)) return -1;
    }
    Q3_HIP(hipStreamSynchronize(v->s), -1);
    return 0;
}

// ---- streaming chunk walk (voc_stream_*) ----
struct StreamState {
    int n_frames = 0;          // frames pushed since the reset
    int n_chunks = 0;          // chunks of the walk decoded and placed
    long long have = 0;        // samples the walk has assembled so far
    long long emitted = 0;     // of which handed out (the rest, have - emitted <= OV, is the device tail)
    bool finished = false;
    int frame_base = 0;        // frames[0] is frame frame_base (earlier ones no future chunk reads)
    std::vector<int64_t> frames;
};

struct VocStream {
    Voc* v = nullptr;
    int max_streams = 0;
    std::vector<StreamState> st;
    float* d_tail = nullptr;          // [max_streams][OV]
    float* d_work = nullptr;          // the push's windows
    size_t work_cap = 0;
    float* d_out = nullptr;           // packed output of a push (f32)
    int16_t* d_out16 = nullptr;       // (int16)
    size_t out_cap = 0, out16_cap = 0;
    StreamWin* d_win = nullptr;       // [max_streams]
    int last_calls = 0, last_chunks = 0;
    float last_ms = 0.f;
};

// What a push would do, worked out without touching the streams: the chunks it decodes (walk[].utt = entry index, dst in the
// stream's own sample coordinates), and per entry the walk's new assembled length and the samples handed out.
struct PushPlan {
    std::vector<WalkChunk> walk;
    std::vector<long long> have, n_out;
    std::vector<int> n_chunks;
};

int plan_push(const VocStream* s, int n, const int32_t* streams, const int32_t* n_new, const int32_t* finish, PushPlan& p) {
    const Voc* v = s->v;
    const int CH = v->chunk;
    const long long OV = 16LL * v->upsample;
    if (n < 0 || (n > 0 && (!streams || !n_new))) return -1;
    p.walk.clear();
    p.have.assign(n, 0);
    p.n_out.assign(n, 0);
    p.n_chunks.assign(n, 0);
    std::vector<char> seen(s->max_streams, 0);
    std::vector<WalkChunk> full;
    for (int i = 0; i < n; i++) {
        const int k = streams[i];
        if (k < 0 || k >= s->max_streams || seen[k] || n_new[i] < 0) {
            Q3_LOG("voc_stream_push: entry %d: bad stream %d (or named twice) or %d new frames", i, k, n_new[i]);
            return -1;
        }
        seen[k] = 1;
        const StreamState& t = s->st[k];
        if (t.finished) {
            Q3_LOG("voc_stream_push: stream %d has finished (voc_stream_reset starts the next utterance)", k);
            return -1;
        }
        const bool fin = finish && finish[i];
        const int N = t.n_frames + n_new[i];
        p.have[i] = t.have;
        p.n_chunks[i] = t.n_chunks;
        if (N > 0) {
            // the walk of the N frames so far; its first chunks are final once all their frames are here (a full chunk whatever
            // follows), the rest only when the utterance ends
            full.clear();
            const long long total = plan_walk(v, i, N, 0, full);
            if (total < 0) return -1;
            int c = t.n_chunks;
            for (; c < (int)full.size() && (fin || full[c].start + CH <= N); c++) {
                p.walk.push_back(full[c]);
                p.have[i] = full[c].dst + (long long)full[c].cl;
            }
            p.n_chunks[i] = c;
            if (fin && p.have[i] != total) return -1;
        }
        p.n_out[i] = fin ? p.have[i] - t.emitted : std::max(0LL, p.have[i] - OV - t.emitted);
    }
    return 0;
}

int stream_push(VocStream* s, int n, const int32_t* streams, const int64_t* codes, const int32_t* n_new, const int32_t* finish,
                bool want16, void* out, int64_t cap, int64_t* offsets) {
    if (!s || !offsets) return -1;
    Voc* v = s->v;
    voc_enter(v);
    const int CH = v->chunk, OV = 16 * v->upsample;
    PushPlan p;
    if (plan_push(s, n, streams, n_new, finish, p)) return -1;
    long long total = 0;
    for (int i = 0; i < n; i++) offsets[i] = total, total += p.n_out[i];
    offsets[n] = total;
    if (total > cap || (total > 0 && !out)) {
        Q3_LOG("voc_stream_push: %lld samples do not fit the caller's buffer of %lld", total, (long long)cap);
        return -1;
    }
    // one window per stream that decodes a chunk or hands samples out: [kept tail | this push's samples]
    std::vector<StreamWin> win;
    std::vector<long long> win_of(n, -1);
    long long work = 0;
    for (int i = 0; i < n; i++) {
        const StreamState& t = s->st[streams[i]];
        const bool fin = finish && finish[i];
        if (p.n_chunks[i] == t.n_chunks && p.n_out[i] == 0) continue;
        const long long size = p.have[i] - t.emitted;
        win_of[i] = work;
        win.push_back({work, offsets[i], p.n_out[i], streams[i], (int)(t.have - t.emitted), fin ? 0 : OV});
        if (!fin && size - p.n_out[i] != OV) return -1;
        work += size;
    }
    for (WalkChunk& c : p.walk) {
        const StreamState& t = s->st[streams[c.utt]];
        if (c.dst < t.emitted || c.dst + (long long)c.cl > p.have[c.utt]) return -1;   // (plan_walk's rules keep every chunk inside)
        c.dst = win_of[c.utt] + (c.dst - t.emitted);
    }
    size_t need = 0;
    for (int i = 0; i < n; i++) need += (size_t)n_new[i];
    if (need > 0 && !codes) return -1;
    // the push is valid: the streams take their new frames
    size_t coff = 0;
    for (int i = 0; i < n; i++) {
        StreamState& t = s->st[streams[i]];
        t.frames.insert(t.frames.end(), codes + coff, codes + coff + (size_t)n_new[i] * 16);
        t.n_frames += n_new[i];
        coff += (size_t)n_new[i] * 16;
    }
    s->last_calls = 0;
    s->last_chunks = (int)p.walk.size();
    s->last_ms = 0.f;
    if (!win.empty()) {
        if (grow(&s->d_work, &s->work_cap, (size_t)work)) return -1;
        Q3_HIP(hipMemcpyAsync(s->d_win, win.data(), sizeof(StreamWin) * win.size(), hipMemcpyHostToDevice, v->s), -1);
        auto load = [&]() -> int { return voc_launch_stream_load(v->s, s->d_tail, OV, s->d_win, s->d_work, (int)win.size()); };
        if (p.walk.empty()) {
            if (load()) return -1;
        } else {
            auto chunk_codes = [&](int c) {
                const WalkChunk& w = p.walk[c];
                const StreamState& t = s->st[streams[w.utt]];
                return t.frames.data() + (size_t)(w.start - t.frame_base) * 16;
            };
            if (decode_walk(v, p.walk, chunk_codes, s->d_work, load, &s->last_calls)) return -1;
            hipEventElapsedTime(&s->last_ms, v->e0, v->e1);
        }
        void* d_out = nullptr;   // (a push that hands nothing out still moves the tails: the f32 kernel without an output)
        if (total > 0) {
            if (want16 ? grow(&s->d_out16, &s->out16_cap, (size_t)total) : grow(&s->d_out, &s->out_cap, (size_t)total)) return -1;
            d_out = want16 ? (void*)s->d_out16 : (void*)s->d_out;
        }
        if (voc_launch_stream_emit(v->s, s->d_work, s->d_win, s->d_tail, OV, d_out, want16 && d_out, (int)win.size())) return -1;
        if (total > 0 && voc_read_back(v, out, d_out, (want16 ? sizeof(int16_t) : sizeof(float)) * (size_t)total)) return -1;
        Q3_HIP(hipStreamSynchronize(v->s), -1);
    }
    for (int i = 0; i < n; i++) {
        StreamState& t = s->st[streams[i]];
        t.have = p.have[i];
        t.emitted += p.n_out[i];
        t.n_chunks = p.n_chunks[i];
        if (finish && finish[i]) {
            t.finished = true;
            std::vector<int64_t>().swap(t.frames);
            continue;
        }
        // the next chunk of the walk starts at frame n_chunks * (CH - 16): earlier frames are never read again
        const int keep_from = t.n_chunks * (CH - 16);
        if (keep_from > t.frame_base) {
            t.frames.erase(t.frames.begin(), t.frames.begin() + (size_t)(keep_from - t.frame_base) * 16);
            t.frame_base = keep_from;
        }
    }
    return 0;
}
}  // namespace

int64_t voc_synthesize_batch_max_samples(void* vv, const int32_t* n_tokens, int U) {
    Voc* v = (Voc*)vv;
    if (!v || !n_tokens || U <= 0) return 0;
    int64_t t = 0;
    for (int u = 0; u < U; u++) t += n_tokens[u] > 0 ? (int64_t)voc_synthesize_max_samples(v, n_tokens[u]) : 0;
    return t;
}

int voc_synthesize_batch_f32(void* vv, const int64_t* codes, const int32_t* n_tokens, int U, float* out, int64_t out_capacity,
                             int64_t* offsets) {
    return synth_batch((Voc*)vv, codes, n_tokens, U, offsets, false, out, out_capacity);
}

int voc_synthesize_batch(void* vv, const int64_t* codes, const int32_t* n_tokens, int U, int16_t* out, int64_t out_capacity,
                         int64_t* offsets) {
    return synth_batch((Voc*)vv, codes, n_tokens, U, offsets, true, out, out_capacity);
}

// one utterance: the batched walk with U = 1
int voc_synthesize_f32(void* vv, const int64_t* codes, int n, float* out, int32_t* n_samples) {
    int64_t offsets[2];
    if (!n_samples || synth_batch((Voc*)vv, codes, &n, 1, offsets, false, out, voc_synthesize_max_samples(vv, n))) return -1;
    *n_samples = (int32_t)offsets[1];
    return 0;
}

int voc_synthesize(void* vv, const int64_t* codes, int n, int16_t* out, int32_t* n_samples) {
    int64_t offsets[2];
    if (!n_samples || synth_batch((Voc*)vv, codes, &n, 1, offsets, true, out, voc_synthesize_max_samples(vv, n))) return -1;
    *n_samples = (int32_t)offsets[1];
    return 0;
}

void* voc_stream_create(void* vv, int max_streams) {
    Voc* v = (Voc*)vv;
    if (!v || max_streams <= 0) return nullptr;
    voc_enter(v);
    VocStream* s = new VocStream;
    s->v = v;
    s->max_streams = max_streams;
    s->st.resize(max_streams);
    const size_t OV = (size_t)16 * v->upsample;
    if (hipMalloc((void**)&s->d_tail, sizeof(float) * OV * max_streams) != hipSuccess ||
        hipMalloc((void**)&s->d_win, sizeof(StreamWin) * max_streams) != hipSuccess) {
        Q3_LOG("voc_stream_create: device allocation failed");
        voc_stream_free(s);
        return nullptr;
    }
    return s;
}

void voc_stream_free(void* ss) {
    VocStream* s = (VocStream*)ss;
    if (!s) return;
    voc_enter(s->v);
    hipStreamSynchronize(s->v->s);
    for (void* p : {(void*)s->d_tail, (void*)s->d_work, (void*)s->d_out, (void*)s->d_out16, (void*)s->d_win})
        if (p) hipFree(p);
    delete s;
}

int voc_stream_reset(void* ss, int stream) {
    VocStream* s = (VocStream*)ss;
    if (!s || stream < 0 || stream >= s->max_streams) return -1;
    s->st[stream] = StreamState();
    return 0;
}

int64_t voc_stream_push_max_samples(void* ss, int n, const int32_t* streams, const int32_t* n_new, const int32_t* finish) {
    VocStream* s = (VocStream*)ss;
    PushPlan p;
    if (!s || plan_push(s, n, streams, n_new, finish, p)) return -1;
    int64_t t = 0;
    for (int i = 0; i < n; i++) t += p.n_out[i];
    return t;
}

int voc_stream_push(void* s, int n, const int32_t* streams, const int64_t* codes, const int32_t* n_new, const int32_t* finish,
                    int16_t* out, int64_t out_capacity, int64_t* offsets) {
    return stream_push((VocStream*)s, n, streams, codes, n_new, finish, true, out, out_capacity, offsets);
}

int voc_stream_push_f32(void* s, int n, const int32_t* streams, const int64_t* codes, const int32_t* n_new, const int32_t* finish,
                        float* out, int64_t out_capacity, int64_t* offsets) {
    return stream_push((VocStream*)s, n, streams, codes, n_new, finish, false, out, out_capacity, offsets);
}

int voc_stream_last_decodes(void* s) { return s ? ((VocStream*)s)->last_calls : -1; }
int voc_stream_last_chunks(void* s) { return s ? ((VocStream*)s)->last_chunks : -1; }
float voc_stream_last_ms(void* s) { return s ? ((VocStream*)s)->last_ms : -1.f; }

float voc_last_batch_ms(void* vv) { return vv ? ((Voc*)vv)->batch_ms : -1.f; }
int voc_last_batch_chunks(void* vv) { return vv ? ((Voc*)vv)->batch_chunks : 0; }

}  // extern "C"

// ---- carry-state incremental decode (voc_incr_*) ----
namespace {

struct VocIncr {
    Voc* v = nullptr;
    int max_streams = 0;
    std::vector<long long> n_frames;      // frames a stream has taken since its reset
    std::vector<char> finished;
    std::vector<int> H;                   // per op: history columns (0: the op carries nothing)
    std::vector<size_t> hoff;             // per op: offset of its [C][H] block inside a stream's state
    size_t state_floats = 0;              // one stream's state
    float* d_hist = nullptr;              // [max_streams][state_floats]
    float* buf[3] = {nullptr, nullptr, nullptr};   // work buffers (voc_run's ping-pong + residual), sized for chunk frames x max_batch
    float* d_kv = nullptr;                // attention: [carried window | new] k and v rows
    int64_t* d_codes = nullptr;           // [max_batch][chunk][16]
    int* d_meta = nullptr;                // [1 + n_ops][max_batch]: the entries' streams, then per op the columns each had consumed
    long long* d_off = nullptr;           // [max_batch]: where each entry's samples start in the packed output
    float* d_out = nullptr;               // packed output of a push
    int16_t* d_out16 = nullptr;
    size_t out_cap = 0;
    DeviceAllocs mem;                     // every device buffer of the object (h_ovf is pinned host memory: incr_destroy)
    float last_ms = 0.f;
    int last_launches = 0;
    // split-fp16 arithmetic (voc_incr_set_arithmetic), allocated by the first switch to it.  The history is then double-buffered:
    // stream k's committed state is d_hist{parity[k]}, a push writes the other buffer and an entry commits by flipping its bit.
    int split = 0;
    size_t buf_elems = 0;                 // floats of one work buffer
    float* d_hist1 = nullptr;
    _Float16* plane[4] = {nullptr, nullptr, nullptr, nullptr};   // two {hi, lo} plane sets, buf_elems halves each
    int* d_par = nullptr;                 // [max_batch]: the entries' parities
    int* d_ovf = nullptr;                 // [max_batch]: an entry's plane value left the fp16 range
    int* h_ovf = nullptr;                 // (pinned)
    std::vector<char> parity;             // per stream
    bool warned_ovf = false;
    int last_split = 0, last_redone = 0;
    float last_restore_ms = 0.f;          // voc_incr_restore
};

int incr_hist_cols(const VocOp& op) {
    switch (op.op) {
        case VOP_CONV: return (op.k - 1) * op.p0;
        case VOP_CONVT: return op.k / op.p0 - 1;      // taps of the polyphase GEMM - 1
        case VOP_DWCONV: return op.k - 1;
        case VOP_ATTN: return op.window - 1;
        default: return 0;
    }
}
int incr_hist_chans(const VocOp& op) { return op.op == VOP_ATTN ? 2 * op.heads * op.head_dim : op.cin; }
// floats of one stream's carried state: the same for every object on a handle (voc_incr_create lays it out op by op)
size_t incr_state_floats(const Voc* v) {
    size_t f = 0;
    for (const VocOp& op : v->ops) f += (size_t)incr_hist_cols(op) * incr_hist_chans(op);
    return f;
}

// in[i]: columns op i has consumed once its stream has taken n frames; in[n_ops]: samples handed out = S(n).  A transposed
// conv whose right trim is k - s (voc_incr_create's rule) turns L columns into L * s - lt: the convt_out chain, 0 where the
// model defines no sample yet.
void incr_chain(const Voc* v, long long n, std::vector<long long>& in) {
    in.resize(v->ops.size() + 1);
    long long L = n;
    for (size_t i = 0; i < v->ops.size(); i++) {
        in[i] = L;
        const VocOp& op = v->ops[i];
        if (op.op == VOP_CONVT) L = std::max(0LL, L * op.p0 - op.lt);
    }
    in[v->ops.size()] = L;
}

// What decides the launches of one entry: per op the new columns it takes (nc, n_ops + 1 values, the last = new samples) and,
// per transposed conv, how many of its first outputs fall before sample 0 (only in a stream's first push).  Entries of a push
// with the same key are decoded together.
void incr_key(const Voc* v, long long prev, long long now, std::vector<long long>& key) {
    std::vector<long long> a, b;
    incr_chain(v, prev, a);
    incr_chain(v, now, b);
    const size_t n = v->ops.size();
    key.assign(2 * n + 1, 0);
    for (size_t i = 0; i <= n; i++) key[i] = b[i] - a[i];
    for (size_t i = 0; i < n; i++)
        if (v->ops[i].op == VOP_CONVT) key[n + 1 + i] = std::max(0LL, (long long)v->ops[i].lt - a[i] * v->ops[i].p0);
}

// One launch sequence: B entries with the same key through the op table: voc_run's branches (the same op -> launch layer,
// q3_voc_program.h) with [history | new] in place of the chunk.  split = false: exact-fp32 kernels only.  split = true: a
// split-capable conv runs launch_conv_split on {hi, lo} planes -- of [history | new] from voc_incr_prepend_split_kernel where it
// carries a history, from its producer's epilogue (voc_run's rule) or voc_launch_snake_split where it carries none -- a residual
// unit runs as its two convs, every other op stays f32; every kernel that writes planes flags its entry in s->d_ovf.
// No launcher rule of the split conv changes the order in which a column's products are summed: conv_split_kernel adds 16-channel
// steps in channel order and taps in tap order inside each, whatever the tile shape (MW, NJ), stage count (KS) and tile order
// (my_fast) launch_conv_split picks from Lc and B -- so nothing needs pinning to the full-chunk length here.  An activation is buf[cur],
// [B][C][pitch4(skip + n)]: `skip` leading columns are the outputs of history columns (dropped: nothing reads them), n are the
// new ones.  dry: no launch, *need / *need_kv take the largest work buffer / k|v buffer (floats per entry) the sequence asks for.
// stop: the walk ends after the first `stop` ops (voc_run's n_ops; the test hook voc_debug_incr_push): the op it ends on hands
// over f32 as the table's last op does, the histories of the ops behind it are not touched.
int incr_walk(VocIncr* s, const std::vector<long long>& key, int B, bool dry, size_t* need, size_t* need_kv, int* launches,
              float** out_buf, int* out_ld, int* out_skip, bool split = false, size_t stop = (size_t)-1) {
    Voc* v = s->v;
    const size_t nops = v->ops.size(), nend = std::min(stop, nops);
    const long long* nc = key.data();
    const long long* extra = key.data() + nops + 1;
    int cur = 0, skip = 0, C = 0;
    long long n = nc[0];
    long Lf = v->chunk;
    float* res = nullptr;
    bool have_res = false;
    int res_ld = -1, res_skip = -1;
    const int mb = v->max_batch;
    auto note = [&](int ch, long long cols) {
        const size_t e = (size_t)ch * pitch4(cols);
        if (need && e > *need) *need = e;
    };
    // buf[cur] columns [skip, skip + n) of channels [c0, c0 + Cc) -> dst = [history | new]; the stream's history moves on
    auto prepend = [&](size_t i, int Cc, int c0, int srcC, float* dst) -> int {
        const int H = s->H[i];
        (*launches)++;
        return dry ? 0 : voc_launch_incr_prepend(v->s, s->buf[cur], srcC, c0, (int)pitch4(skip + n), skip, dst, Cc, (int)pitch4(H + n),
                                                 s->d_hist + s->hoff[i], s->d_hist1 ? s->d_hist1 + s->hoff[i] : nullptr,
                                                 s->d_hist1 ? s->d_par : nullptr, H, (int)n, (long long)s->state_floats, s->d_meta, B);
    };
    int planes = -1;          // split: the plane set that holds the current activation in its consumer's input form, or -1
    bool f32_cur = true;      // split: buf[cur] holds the current activation
    auto prepend_act = [&](size_t i) -> int {     // the whole activation: it becomes buf[cur] = [history | new]
        if (s->H[i] == 0) return 0;
        note(C, s->H[i] + n);
        if (prepend(i, C, 0, C, dry ? nullptr : s->buf[cur ^ 1])) return -1;
        cur ^= 1;
        skip = s->H[i];
        return 0;
    };
    auto save_res = [&]() {                       // voc_run: the unit's input becomes buf[2], out of the ping-pong
        std::swap(s->buf[2], s->buf[cur]);
        res = s->buf[2];
        have_res = true;
        res_ld = (int)pitch4(skip + n);
        res_skip = skip;
    };
    size_t i = 0;
    for (; i < nend; i++) {
        const VocOp& op = v->ops[i];
        if (n != nc[i]) return -1;
        if (n == 0) break;                        // no sample of this push reaches further (a stream's very first columns)
        if (!f32_cur && !(split && voc_split_capable(op))) return -1;   // only a split conv reads planes
        if (op.op == VOP_RVQ || op.op == VOP_EMBMEAN) {
            note(op.cout, n);
            if (!dry && voc_op_embed(v, op, s->d_codes, s->buf[cur ^ 1], (int)n, B)) return -1;
            skip = 0;
        } else if (op.op == VOP_DWCONV || op.op == VOP_NORM || op.op == VOP_GLU) {
            if (op.op == VOP_DWCONV && prepend_act(i)) return -1;
            if (op.flags & VF_RES_SAVE) save_res();
            note(op.cout, skip + n);
            if (!dry && voc_op_pointwise(v, op, (op.flags & VF_RES_SAVE) ? res : s->buf[cur], s->buf[cur ^ 1], skip + n, B)) return -1;
        } else if (op.op == VOP_ATTN) {
            // k | v rows of the new columns join the carried window in d_kv; q stays where it is, the output keeps the
            // input's columns (the residual saved before the q/k/v projection lines up with it)
            const int HD = op.heads * op.head_dim, Hk = s->H[i];
            if (need_kv) *need_kv = std::max(*need_kv, (size_t)2 * HD * pitch4(Hk + n));
            if (prepend(i, 2 * HD, HD, 3 * HD, dry ? nullptr : s->d_kv)) return -1;
            note(HD, skip + n);
            if (!dry && voc_launch_incr_attn(v->s, s->buf[cur], (int)pitch4(skip + n), skip, s->d_kv, (int)pitch4(Hk + n), Hk, s->buf[cur ^ 1],
                                             op.heads, op.head_dim, op.window, op.theta, s->d_meta + (1 + i) * mb, (int)n, B))
                return -1;
        } else if (split && voc_split_capable(op)) {
            const int H = s->H[i];
            int in_set = planes;
            if (H > 0) {
                // [history | new] straight into the planes; as f32 too where it is the unit's residual
                if (!f32_cur) return -1;
                const bool keep = (op.flags & VF_RES_SAVE) != 0;
                in_set = 0;
                note(C, H + n);
                if (!dry && voc_launch_incr_prepend_split(v->s, s->buf[cur], (int)pitch4(skip + n), skip, s->plane[0], s->plane[1],
                                                  keep ? s->buf[cur ^ 1] : nullptr, (int)pitch4(H + n), C, op.alpha, op.inv_beta,
                                                  (op.flags & VF_GELU) ? 1 : 0, s->d_hist + s->hoff[i], s->d_hist1 + s->hoff[i], s->d_par, H,
                                                  (int)n, (long long)s->state_floats, s->d_meta, s->d_ovf, B))
                    return -1;
                (*launches)++;
                if (keep) cur ^= 1;
                skip = H;
            } else if (in_set < 0) {
                if (!f32_cur) return -1;
                in_set = 0;
                // (over the skip leading columns too: nothing reads their planes, but they can raise the entry's flag -- a redo
                // that was not needed is exact all the same; include/qwen3tts_voc.h)
                if (!dry && voc_launch_snake_split(v->s, s->buf[cur], op.alpha, op.inv_beta, s->plane[0], s->plane[1], C, (int)(skip + n),
                                           (int)pitch4(skip + n), (op.flags & VF_GELU) ? 1 : 0, s->d_ovf, B, 1))
                    return -1;
                (*launches)++;
            }
            if (op.flags & VF_RES_SAVE) {
                if (!f32_cur) return -1;     // (the producer keeps an f32 copy whenever its consumer saves a residual)
                save_res();
            }
            const long long cols = skip + n;
            SplitArgs sa = voc_split_args(op, cols);
            long long n_next = n;
            int skip_next = skip;
            if (op.op == VOP_CONVT) {        // the exact branch's geometry, see below
                n_next = nc[i + 1];
                skip_next = 0;
                sa.lt = skip * op.p0 + (int)extra[i];
                sa.Lout = (int)n_next;
                sa.Lc = (int)cols;
                sa.ldy = (int)pitch4(sa.Lout);
                Lf = convt_out(op, Lf);
                if (n_next == 0) {
                    n = 0;
                    i++;
                    break;
                }
            }
            note(op.cout, sa.Lout);
            // the consumer takes planes from this epilogue only where it reads these very columns: one that carries a history
            // needs the f32 result for its own prepend
            const VocOp* next = i + 1 < nend ? &v->ops[i + 1] : nullptr;
            const bool want_planes = voc_split_emits_planes(op, next) && s->H[i + 1] == 0;
            const bool want_f32 = !want_planes || (next->flags & VF_RES_SAVE);
            if (op.flags & VF_RES_ADD) {
                if (!have_res || res_ld != sa.ldy || res_skip != skip_next || op.op != VOP_CONV) {
                    Q3_LOG("voc incremental: op %zu adds a residual that is not aligned with its output", i);
                    return -1;
                }
                sa.res = res;
            }
            sa.xh = s->plane[2 * in_set];
            sa.xl = s->plane[2 * in_set + 1];
            sa.ovf = s->d_ovf;
            sa.ovf_stride = 1;
            if (want_f32) sa.y = s->buf[cur ^ 1];
            if (want_planes) voc_split_out_planes(sa, *next, s->plane[2 * (in_set ^ 1)], s->plane[2 * (in_set ^ 1) + 1]);
            if (want_planes) note(op.cout, cols);
            if (!dry && launch_conv_split(v->s, sa, voc_split_taps(op), B, v->cfg)) return -1;
            if (!dry) s->last_split++;
            f32_cur = want_f32;
            planes = want_planes ? (in_set ^ 1) : -1;
            n = n_next;
            skip = skip_next;
            (*launches)++;
            C = op.cout;
            cur ^= 1;
            continue;
        } else if (!split && voc_fused_unit(v, i, nend)) {
            if (prepend_act(i)) return -1;
            if (!dry && launch_resunit(v->s, voc_resunit_args(op, v->ops[i + 1], s->buf[cur], s->buf[cur ^ 1], skip + n), op.cin, B, v->cfg)) return -1;
            i++;   // the 1x1 conv is done
            if (nc[i] != n) return -1;
        } else {
            if (prepend_act(i)) return -1;
            if (op.flags & VF_RES_SAVE) save_res();
            const long long cols = skip + n;
            ConvArgs a = voc_conv_args(op, cols, Lf);
            long long n_next = n;
            int skip_next = skip;
            if (op.op == VOP_CONVT) {
                // buffer column skip + j is the stream's column prev + j; its virtual row p is the stream's output sample
                // (prev + j) * s + p - lt, i.e. new sample number (skip + j) * s + p - a.lt of this push: the stream's trim, this
                // push's samples and every column it holds stand in for the whole-chunk geometry
                n_next = nc[i + 1];
                skip_next = 0;
                a.lt = skip * op.p0 + (int)extra[i];
                a.Lout = (int)n_next;
                a.Lc = (int)cols;
                a.ldy = (int)pitch4(a.Lout);
                Lf = convt_out(op, Lf);
                if (n_next == 0) {   // every output of these columns lies before sample 0: the history has moved on, nothing to compute
                    n = 0;
                    i++;
                    break;
                }
            }
            note(op.cout, a.Lout);
            if (op.flags & VF_RES_ADD) {
                if (!have_res || res_ld != a.ldy || res_skip != skip_next || op.op != VOP_CONV) {
                    Q3_LOG("voc incremental: op %zu adds a residual that is not aligned with its output", i);
                    return -1;
                }
                a.res = res;
            }
            a.x = (op.flags & VF_RES_SAVE) ? res : s->buf[cur];
            a.y = s->buf[cur ^ 1];
            if (!dry && voc_launch_conv(v->s, a, B, v->cfg)) return -1;
            n = n_next;
            skip = skip_next;
        }
        (*launches)++;
        C = op.cout;
        cur ^= 1;
        planes = -1;
    }
    if (i == nops && n != nc[nops]) return -1;
    if (i < nend && nc[nops] != 0) return -1;
    if (!f32_cur && n > 0) return -1;
    if (out_buf) *out_buf = s->buf[cur];
    if (out_ld) *out_ld = (int)pitch4(skip + n);
    if (out_skip) *out_skip = skip;
    return 0;
}

struct IncrPlan {
    std::vector<long long> n_out;   // per entry
    PushGroups groups;              // keys: incr_key
};

int incr_plan(const VocIncr* s, int n, const int32_t* streams, const int32_t* n_new, IncrPlan& p) {
    const Voc* v = s->v;
    if (n < 0 || (n > 0 && (!streams || !n_new))) return -1;
    p.n_out.assign(n, 0);
    p.groups = PushGroups();
    std::vector<char> seen(s->max_streams, 0);
    std::vector<long long> key;
    const size_t nops = v->ops.size();
    for (int i = 0; i < n; i++) {
        const int k = streams[i];
        if (k < 0 || k >= s->max_streams || seen[k] || n_new[i] < 0 || n_new[i] > v->chunk) {
            Q3_LOG("voc_incr_push: entry %d: bad stream %d (or named twice) or %d new frames (0..%d)", i, k, n_new[i], v->chunk);
            return -1;
        }
        seen[k] = 1;
        if (s->finished[k]) {
            Q3_LOG("voc_incr_push: stream %d has finished (voc_incr_reset starts the next utterance)", k);
            return -1;
        }
        if (n_new[i] == 0) continue;      // (a finish push adds no sample: the model defines nothing past S(N))
        if (s->n_frames[k] + n_new[i] > 0x7fffffffLL) {
            Q3_LOG("voc_incr_push: stream %d is beyond 2^31 frames", k);
            return -1;
        }
        incr_key(v, s->n_frames[k], s->n_frames[k] + n_new[i], key);
        p.n_out[i] = key[nops];
        p.groups.add(key, i, v->max_batch);
    }
    return 0;
}

// n_stop >= 0 (voc_debug_incr_push): the walk ends after the first n_stop ops and `out` (f32) takes, per entry, the new columns
// of that activation, [C][cols] packed at offsets[e] (floats), straight from the work buffer; *out_C = C.
int incr_push(VocIncr* s, int n, const int32_t* streams, const int64_t* codes, const int32_t* n_new, const int32_t* finish,
              bool want16, void* out, int64_t cap, int64_t* offsets, int n_stop = -1, int32_t* out_C = nullptr) {
    if (!s || !offsets) return -1;
    Voc* v = s->v;
    voc_enter(v);
    IncrPlan p;
    if (incr_plan(s, n, streams, n_new, p)) return -1;
    const bool debug = n_stop >= 0;
    const size_t stop = debug ? std::min((size_t)n_stop, v->ops.size()) : v->ops.size();
    const int stop_C = stop > 0 ? v->ops[stop - 1].cout : 0;
    if (debug) {
        if (want16 || stop == 0) return -1;
        for (size_t g = 0; g < p.groups.keys.size(); g++)
            for (int e : p.groups.members[g]) p.n_out[e] = p.groups.keys[g][stop] * stop_C;
        if (out_C) *out_C = stop_C;
    }
    long long total = 0;
    size_t frames = 0;
    std::vector<size_t> coff(n, 0);
    for (int i = 0; i < n; i++) {
        offsets[i] = total;
        total += p.n_out[i];
        coff[i] = frames * 16;
        frames += (size_t)n_new[i];
    }
    offsets[n] = total;
    if (total > cap || (total > 0 && !out) || (frames > 0 && !codes) || (!debug && (size_t)total > s->out_cap)) {
        Q3_LOG("voc_incr_push: %lld samples do not fit the caller's buffer of %lld (or no codes given)", total, (long long)cap);
        return -1;
    }
    // the push is valid
    const size_t nops = v->ops.size();
    const int mb = v->max_batch;
    std::vector<int64_t> hcodes;
    std::vector<int> meta((1 + nops) * mb);
    std::vector<long long> off(mb), before;
    std::vector<int> par(mb);
    s->last_launches = 0;
    s->last_ms = 0.f;
    s->last_split = 0;
    s->last_redone = 0;
    if (!p.groups.keys.empty()) Q3_HIP(hipEventRecord(v->e0, v->s), -1);
    // one launch sequence over the entries `mem` of a group, on the split or the exact branch, complete on return
    auto run_group = [&](const std::vector<long long>& key, const std::vector<int>& mem, bool split) -> int {
        const int B = (int)mem.size(), T = n_new[mem[0]];
        hcodes.resize((size_t)B * T * 16);
        std::fill(meta.begin(), meta.end(), 0);
        for (int b = 0; b < B; b++) {
            const int e = mem[b], k = streams[e];
            memcpy(hcodes.data() + (size_t)b * T * 16, codes + coff[e], sizeof(int64_t) * 16 * T);
            incr_chain(v, s->n_frames[k], before);
            meta[b] = k;
            for (size_t i = 0; i < nops; i++) meta[(1 + i) * mb + b] = (int)before[i];
            off[b] = offsets[e];
            if (s->d_hist1) par[b] = s->parity[k];
        }
        Q3_HIP(hipMemcpyAsync(s->d_codes, hcodes.data(), sizeof(int64_t) * hcodes.size(), hipMemcpyHostToDevice, v->s), -1);
        Q3_HIP(hipMemcpyAsync(s->d_meta, meta.data(), sizeof(int) * meta.size(), hipMemcpyHostToDevice, v->s), -1);
        Q3_HIP(hipMemcpyAsync(s->d_off, off.data(), sizeof(long long) * B, hipMemcpyHostToDevice, v->s), -1);
        if (s->d_hist1) Q3_HIP(hipMemcpyAsync(s->d_par, par.data(), sizeof(int) * B, hipMemcpyHostToDevice, v->s), -1);
        if (split) Q3_HIP(hipMemsetAsync(s->d_ovf, 0, sizeof(int) * B, v->s), -1);
        float* y = nullptr;
        int ld = 0, skip = 0;
        if (incr_walk(s, key, B, false, nullptr, nullptr, &s->last_launches, &y, &ld, &skip, split, stop)) return -1;
        const long long ns = debug ? 0 : key[nops];
        if (debug && key[stop] > 0) {   // rows of key[stop] new columns behind the `skip` dropped ones -> the caller's packed block
            const size_t row = sizeof(float) * (size_t)key[stop];
            for (int b = 0; b < B; b++)
                Q3_HIP(hipMemcpy2DAsync((float*)out + offsets[mem[b]], row, y + (size_t)b * stop_C * ld + skip, sizeof(float) * (size_t)ld, row,
                                        (size_t)stop_C, hipMemcpyDeviceToHost, v->s), -1);
        }
        if (ns > 0) {
            if (voc_launch_incr_emit(v->s, y, ld, skip, (int)ns, s->d_off, want16 ? (void*)s->d_out16 : (void*)s->d_out, want16, B)) return -1;
            s->last_launches++;
        }
        if (split) Q3_HIP(hipMemcpyAsync(s->h_ovf, s->d_ovf, sizeof(int) * B, hipMemcpyDeviceToHost, v->s), -1);
        Q3_HIP(hipStreamSynchronize(v->s), -1);   // the staging vectors are reused by the next group
        return 0;
    };
    std::vector<int> redo;
    for (size_t g = 0; g < p.groups.keys.size(); g++) {
        const std::vector<int>& mem = p.groups.members[g];
        if (run_group(p.groups.keys[g], mem, s->split != 0)) return -1;
        if (s->split) {
            // a push is a transaction per entry: an entry whose planes left the fp16 range is not committed -- the flagged
            // entries of the group run again, from their uncommitted history, on the exact branch, and their samples replace the
            // split ones; the others' bits never depended on them (every kernel works per entry)
            redo.clear();
            for (size_t b = 0; b < mem.size(); b++)
                if (s->h_ovf[b]) redo.push_back(mem[b]);
            if (!redo.empty()) {
                if (!s->warned_ovf)
                    Q3_LOG("vocoder incremental: activation outside the fp16 range, decoding this entry's push with the exact-fp32 path");
                s->warned_ovf = true;
                if (run_group(p.groups.keys[g], redo, false)) return -1;
                s->last_redone += (int)redo.size();
            }
        }
        if (s->d_hist1)
            for (int e : mem) s->parity[streams[e]] ^= 1;   // commit: the written buffer is the stream's history now
    }
    if (!p.groups.keys.empty()) {
        Q3_HIP(hipEventRecord(v->e1, v->s), -1);
        if (total > 0 && !debug)
            if (voc_read_back(v, out, want16 ? (void*)s->d_out16 : (void*)s->d_out, (want16 ? sizeof(int16_t) : sizeof(float)) * (size_t)total))
                return -1;
        Q3_HIP(hipStreamSynchronize(v->s), -1);
        hipEventElapsedTime(&s->last_ms, v->e0, v->e1);
    }
    for (int i = 0; i < n; i++) {
        s->n_frames[streams[i]] += n_new[i];
        if (finish && finish[i]) s->finished[streams[i]] = 1;
    }
    return 0;
}

void incr_destroy(VocIncr* s) {
    if (!s) return;
    if (s->h_ovf) hipHostFree(s->h_ovf);
    delete s;   // (its device allocations go with it: DeviceAllocs)
}
}  // namespace

extern "C" {

int64_t voc_incr_samples(void* vv, int64_t n_frames) {
    const Voc* v = (const Voc*)vv;
    if (!v || n_frames < 0) return -1;
    std::vector<long long> in;
    incr_chain(v, n_frames, in);
    return in.back();
}

void voc_incr_free(void* ss) {
    VocIncr* s = (VocIncr*)ss;
    if (!s) return;
    voc_enter(s->v);
    hipStreamSynchronize(s->v->s);
    incr_destroy(s);
}

void* voc_incr_create(void* vv, int max_streams) {
    Voc* v = (Voc*)vv;
    if (!v || max_streams <= 0) return nullptr;
    voc_enter(v);
    VocIncr* s = new VocIncr;
    s->v = v;
    s->max_streams = max_streams;
    s->n_frames.assign(max_streams, 0);
    s->finished.assign(max_streams, 0);
    s->parity.assign(max_streams, 0);
    const size_t nops = v->ops.size();
    s->H.assign(nops, 0);
    s->hoff.assign(nops, 0);
    for (size_t i = 0; i < nops; i++) {
        const VocOp& op = v->ops[i];
        // a stream can only run on a table whose transposed convs never emit a sample that a later column changes: the right
        // trim takes the k - s outputs the next input column still adds to ('both' and 'right' trims, and k = s untrimmed)
        if (op.op == VOP_CONVT && (op.rt != op.k - op.p0 || op.lt > op.p0)) {
            Q3_LOG("voc_incr_create: op %zu: a transposed conv k=%d s=%d trimmed %d + %d cannot be streamed (right trim must be k - s)", i,
                   op.k, op.p0, op.lt, op.rt);
            delete s;
            return nullptr;
        }
        s->H[i] = incr_hist_cols(op);
        if (s->H[i] > 256 || (op.op == VOP_ATTN && op.head_dim > 128)) {
            Q3_LOG("voc_incr_create: op %zu carries %d columns, more than the 256 the history kernel holds", i, s->H[i]);
            delete s;
            return nullptr;
        }
        s->hoff[i] = s->state_floats;
        s->state_floats += (size_t)s->H[i] * incr_hist_chans(op);
    }
    // work buffers: the largest activation [history | new] of a push of chunk_tokens frames, first push or later
    size_t need = 0, need_kv = 0;
    std::vector<long long> key;
    bool ok = true;
    for (long long prev : {0LL, (long long)v->chunk}) {
        int launches = 0;
        incr_key(v, prev, prev + v->chunk, key);
        ok = ok && incr_walk(s, key, v->max_batch, true, &need, &need_kv, &launches, nullptr, nullptr, nullptr) == 0;
    }
    if (!ok) {
        Q3_LOG("voc_incr_create: the vocoder program cannot be run incrementally");
        delete s;
        return nullptr;
    }
    const size_t mb = (size_t)v->max_batch;
    const size_t buf_elems = need * mb + 1024, kv_elems = need_kv * mb + 1024;   // (+ slack: float4 groups past a row's last column)
    s->buf_elems = buf_elems;
    s->out_cap = (size_t)max_streams * v->chunk * v->upsample;
    DeviceAllocs& m = s->mem;
    ok = m.alloc_zeroed(&s->d_hist, sizeof(float) * std::max<size_t>(1, s->state_floats * max_streams), v->s);
    for (int i = 0; i < 3; i++) ok = ok && m.alloc_zeroed(&s->buf[i], sizeof(float) * buf_elems, v->s);   // (zeroed once: dropped columns start finite)
    ok = ok && m.alloc_zeroed(&s->d_kv, sizeof(float) * kv_elems, v->s) && m.alloc(&s->d_codes, sizeof(int64_t) * 16 * v->chunk * mb) &&
         m.alloc(&s->d_meta, sizeof(int) * (1 + nops) * mb) && m.alloc(&s->d_off, sizeof(long long) * mb) &&
         m.alloc(&s->d_out, sizeof(float) * s->out_cap) && m.alloc(&s->d_out16, sizeof(int16_t) * s->out_cap) &&
         hipStreamSynchronize(v->s) == hipSuccess;   // the zeroing above
    if (!ok) {
        Q3_LOG("voc_incr_create: device allocation failed");
        incr_destroy(s);
        return nullptr;
    }
    return s;
}

int voc_incr_reset(void* ss, int stream) {
    VocIncr* s = (VocIncr*)ss;
    if (!s || stream < 0 || stream >= s->max_streams) return -1;
    voc_enter(s->v);
    if (s->state_floats)   // the stream's history is the zero padding again (ordered before the next push on the handle's stream)
        Q3_HIP(hipMemsetAsync(s->d_hist + (size_t)stream * s->state_floats, 0, sizeof(float) * s->state_floats, s->v->s), -1);
    if (s->state_floats && s->d_hist1)   // (both buffers: an op a short first push does not reach reads the other one next time)
        Q3_HIP(hipMemsetAsync(s->d_hist1 + (size_t)stream * s->state_floats, 0, sizeof(float) * s->state_floats, s->v->s), -1);
    s->parity[stream] = 0;
    s->n_frames[stream] = 0;
    s->finished[stream] = 0;
    return 0;
}

int64_t voc_incr_push_max_samples(void* ss, int n, const int32_t* streams, const int32_t* n_new, const int32_t* finish) {
    VocIncr* s = (VocIncr*)ss;
    IncrPlan p;
    if (!s || incr_plan(s, n, streams, n_new, p)) return -1;
    int64_t t = 0;
    for (int i = 0; i < n; i++) t += p.n_out[i];
    return t;
}

int voc_incr_push(void* s, int n, const int32_t* streams, const int64_t* codes, const int32_t* n_new, const int32_t* finish,
                  int16_t* out, int64_t out_capacity, int64_t* offsets) {
    return incr_push((VocIncr*)s, n, streams, codes, n_new, finish, true, out, out_capacity, offsets);
}

int voc_incr_push_f32(void* s, int n, const int32_t* streams, const int64_t* codes, const int32_t* n_new, const int32_t* finish,
                      float* out, int64_t out_capacity, int64_t* offsets) {
    return incr_push((VocIncr*)s, n, streams, codes, n_new, finish, false, out, out_capacity, offsets);
}

// test hook (like voc_debug_run, not in the header): a push whose walk ends after the first n_ops ops.  out takes, per entry, the
// new columns of that activation, [C][cols] f32 packed at offsets[e] (offsets[n] = the total, in floats); *C its channels.  The
// histories of the ops that ran move on exactly as in a real push, later ops' are not touched: a stream driven through this hook
// is reset (voc_incr_reset) before it is driven through voc_incr_push*.
int voc_debug_incr_push(void* s, int n, const int32_t* streams, const int64_t* codes, const int32_t* n_new, int n_ops, float* out,
                        int64_t out_capacity, int64_t* offsets, int32_t* C) {
    if (n_ops <= 0) return -1;
    return incr_push((VocIncr*)s, n, streams, codes, n_new, nullptr, false, out, out_capacity, offsets, n_ops, C);
}

float voc_incr_last_ms(void* s) { return s ? ((VocIncr*)s)->last_ms : -1.f; }
int voc_incr_last_launches(void* s) { return s ? ((VocIncr*)s)->last_launches : -1; }
int64_t voc_incr_state_bytes(void* s) { return s ? (int64_t)(((VocIncr*)s)->state_floats * sizeof(float)) : -1; }
int64_t voc_incr_device_bytes(void* s) { return s ? (int64_t)((VocIncr*)s)->mem.bytes : -1; }

int voc_incr_set_arithmetic(void* ss, int split) {
    VocIncr* s = (VocIncr*)ss;
    if (!s || (split != 0 && split != 1)) return -1;
    for (int k = 0; k < s->max_streams; k++)
        if (s->n_frames[k] > 0 && !s->finished[k]) {
            Q3_LOG("voc_incr_set_arithmetic: stream %d is running (the arithmetic changes between utterances only)", k);
            return -1;
        }
    if (split && !s->d_hist1) {
        Voc* v = s->v;
        voc_enter(v);
        // the split walk's activations and planes must fit what voc_incr_create sized from the exact walk (the same ops over the
        // same columns: a table where they do not is refused here, not overrun)
        size_t need = 0, need_kv = 0;
        std::vector<long long> key;
        for (long long prev : {0LL, (long long)s->v->chunk}) {
            int launches = 0;
            incr_key(s->v, prev, prev + s->v->chunk, key);
            if (incr_walk(s, key, s->v->max_batch, true, &need, &need_kv, &launches, nullptr, nullptr, nullptr, true) ||
                need * (size_t)s->v->max_batch + 1024 > s->buf_elems) {
                Q3_LOG("voc_incr_set_arithmetic: the split walk does not fit the object's work buffers");
                return -1;
            }
        }
        // the second history buffer, the plane sets and the per-entry flags.  Every stream is idle, and an idle stream's next
        // utterance starts with voc_incr_reset (or is the first of a fresh object): both buffers zero, parity 0.
        const size_t mb = (size_t)v->max_batch, hist = sizeof(float) * std::max<size_t>(1, s->state_floats * s->max_streams);
        DeviceAllocs got;   // all or nothing: the object adopts it once every buffer is there and filled
        float* hist1 = nullptr;
        _Float16* plane[4] = {nullptr, nullptr, nullptr, nullptr};
        int *par = nullptr, *ovf = nullptr, *h = nullptr;
        bool ok = hipHostMalloc((void**)&h, sizeof(int) * mb, 0) == hipSuccess && got.alloc(&hist1, hist);
        for (int i = 0; i < 4; i++) ok = ok && got.alloc_zeroed(&plane[i], sizeof(_Float16) * s->buf_elems, v->s);
        // the history a fresh stream continues from is zero in both buffers (a stream that ran in exact mode and finished is reset
        // before its next utterance, which zeroes both)
        ok = ok && got.alloc(&par, sizeof(int) * mb) && got.alloc(&ovf, sizeof(int) * mb) &&
             hipMemcpyAsync(hist1, s->d_hist, hist, hipMemcpyDeviceToDevice, v->s) == hipSuccess && hipStreamSynchronize(v->s) == hipSuccess;
        if (!ok) {
            Q3_LOG("voc_incr_set_arithmetic: device allocation failed");
            if (h) hipHostFree(h);
            return -1;   // (`got` frees what it had)
        }
        s->mem.adopt(got);
        s->d_hist1 = hist1;
        std::copy(plane, plane + 4, s->plane);
        s->d_par = par;
        s->d_ovf = ovf;
        s->h_ovf = h;
    }
    s->split = split;
    return s->split;
}

int voc_incr_arithmetic(void* s) { return s ? ((VocIncr*)s)->split : -1; }
int voc_incr_last_split_launches(void* s) { return s ? ((VocIncr*)s)->last_split : -1; }
int voc_incr_last_redone(void* s) { return s ? ((VocIncr*)s)->last_redone : -1; }

// ---- snapshots of a stream's carried state (the pool is the handle's: q3_voc_program.h) ----
int voc_incr_snapshots(void* vv, int n_slots) {
    Voc* v = (Voc*)vv;
    if (!v || n_slots < 0) return -1;
    voc_enter(v);
    float* pool = nullptr;
    const size_t pitch = (incr_state_floats(v) + 3) / 4 * 4;
    if (n_slots > 0 && hipMalloc((void**)&pool, sizeof(float) * std::max<size_t>(4, pitch * (size_t)n_slots)) != hipSuccess) {
        Q3_LOG("voc_incr_snapshots: no device memory for %d slots of %zu bytes", n_slots, sizeof(float) * pitch);
        return -1;
    }
    hipStreamSynchronize(v->s);   // (a save or restore of the old pool is complete before it goes)
    if (v->d_snap) hipFree(v->d_snap);
    v->d_snap = pool;
    v->snap_pitch = pitch;
    v->snap_frames.assign(n_slots, -1);
    v->snap_split.assign(n_slots, 0);
    return n_slots;
}

int64_t voc_incr_snapshot_frames(void* vv, int slot) {
    const Voc* v = (const Voc*)vv;
    if (!v || slot < 0 || slot >= (int)v->snap_frames.size()) return -1;
    return v->snap_frames[slot];
}

int voc_incr_save(void* ss, int stream, int slot) {
    VocIncr* s = (VocIncr*)ss;
    if (!s || stream < 0 || stream >= s->max_streams || s->finished[stream]) return -1;
    Voc* v = s->v;
    if (!v->d_snap || slot < 0 || slot >= (int)v->snap_frames.size()) return -1;
    voc_enter(v);
    // the committed history: in a double-buffered object the buffer the stream's parity selects
    const float* hist = (s->d_hist1 && s->parity[stream] ? s->d_hist1 : s->d_hist) + (size_t)stream * s->state_floats;
    if (s->state_floats)
        Q3_HIP(hipMemcpyAsync(v->d_snap + (size_t)slot * v->snap_pitch, hist, sizeof(float) * s->state_floats, hipMemcpyDeviceToDevice, v->s), -1);
    v->snap_frames[slot] = s->n_frames[stream];
    v->snap_split[slot] = (char)s->split;
    return 0;
}

int voc_incr_restore(void* ss, int n, const int32_t* streams, const int32_t* slots) {
    VocIncr* s = (VocIncr*)ss;
    if (!s || n < 0 || (n > 0 && (!streams || !slots))) return -1;
    Voc* v = s->v;
    if (!v->d_snap) {
        Q3_LOG("voc_incr_restore: the handle has no snapshot pool (voc_incr_snapshots)");
        return -1;
    }
    // every entry is checked before any stream changes
    std::vector<char> seen(s->max_streams, 0);
    for (int i = 0; i < n; i++) {
        const int k = streams[i], z = slots[i];
        if (k < 0 || k >= s->max_streams || seen[k] || z < 0 || z >= (int)v->snap_frames.size() || v->snap_frames[z] < 0) {
            Q3_LOG("voc_incr_restore: entry %d: bad stream %d (or named twice) or bad or empty slot %d", i, k, z);
            return -1;
        }
        if (v->snap_split[z] != (char)s->split) {
            Q3_LOG("voc_incr_restore: slot %d was saved under the %s arithmetic, the object runs the %s one", z,
                   v->snap_split[z] ? "split" : "exact", s->split ? "split" : "exact");
            return -1;
        }
        seen[k] = 1;
    }
    s->last_restore_ms = 0.f;
    if (n == 0) return 0;
    voc_enter(v);
    if (grow(&v->d_snap_tab, &v->snap_tab_cap, (size_t)std::max(n, s->max_streams))) return -1;
    std::vector<SnapCopy> tab(n);
    for (int i = 0; i < n; i++) {
        const size_t ho = (size_t)streams[i] * s->state_floats;
        tab[i] = {v->d_snap + (size_t)slots[i] * v->snap_pitch, s->d_hist + ho, s->d_hist1 ? s->d_hist1 + ho : nullptr};
    }
    Q3_HIP(hipMemcpyAsync(v->d_snap_tab, tab.data(), sizeof(SnapCopy) * n, hipMemcpyHostToDevice, v->s), -1);
    Q3_HIP(hipEventRecord(v->e0, v->s), -1);
    if (s->state_floats && voc_launch_incr_restore(v->s, v->d_snap_tab, (long long)s->state_floats, n)) return -1;
    Q3_HIP(hipEventRecord(v->e1, v->s), -1);
    Q3_HIP(hipStreamSynchronize(v->s), -1);   // (the table's staging vector; the events)
    hipEventElapsedTime(&s->last_restore_ms, v->e0, v->e1);
    for (int i = 0; i < n; i++) {
        const int k = streams[i];
        s->parity[k] = 0;   // both buffers hold the slot's columns
        s->n_frames[k] = v->snap_frames[slots[i]];
        s->finished[k] = 0;
    }
    return 0;
}

float voc_incr_last_restore_ms(void* s) { return s ? ((VocIncr*)s)->last_restore_ms : -1.f; }

}  // extern "C"
