// q3_enc_stream_pcm.hip -- the streaming encode's PCM front-end for gfx950 (enc_stream_push_pcm,
// include/qwen3tts_enc_stream_pcm.h): a push of interleaved s16le / f32le PCM of 1..8 channels at a client's rate -> the 24 kHz
// mono f32 samples its frames have settled, written into the rows of EncStream::d_pcm that enc_stream_push's walk reads.  The
// arithmetic is enc_encode_pcm's (q3_enc_pcm.hip, q3_enc_pcm_host.h): the same taps, the same float64 fma chain per output,
// rounded once -- over the same operands, because a stream carries the J - 1 downmixed frames (doubles) that the first
// output of its next push still reaches back to (q3_enc_stream_pcm_host.h).  So a stream's samples are the bits of
// enc_encode_pcm's for any split of the clip, and its ids those of enc_stream_push fed these samples.
//
// enc_stream_pcm_kernel, one launch per group of a push (grid: 256 outputs x member), has enc_pcm_kernel's shape: the taps
// [J][up] and the workgroup's window of input frames in LDS as doubles, a bounds-free inner loop.  The window is filled by
// absolute frame index i: zero for i < 0 and from the stream's total on (what the whole-clip kernel pads with; only outputs of
// a finishing push reach there), the stream's carry row for frames before this push, the decoded and downmixed wire payload
// for this push's frames.  Output m of the stream lands in column m - ready(frames before the push) of the member's row.
//
// enc_stream_pcm_carry_kernel, one launch per push after every resample launch: the last J - 1 frames of [old carry | new
// frames] become the carry.  A stream has two rows and the kernel writes the one the push did not read (the host flips them
// when the push has succeeded), so no workgroup reads what another writes and a refused or failed push leaves the carry whole.
#include "../../include/qwen3tts_enc.h"
#include "q3_enc.h"
#include "q3_enc_stream_pcm_host.h"

#include <algorithm>
#include <cmath>

namespace q3 {

constexpr int ENC_SPCM_OUTPUTS = 256;   // per workgroup, one per thread
constexpr int ENC_SPCM_META = 8;        // long longs per entry: payload frame, frames before, frames after, first output,
                                        // outputs, carry row read, carry row written, (unused)

struct EncStreamPcm {
    std::vector<long long> total_in;    // input frames a stream has taken since its reset
    std::vector<int> format, channels, rate;   // of the clip's first push
    std::vector<char> half;             // which of the stream's two carry rows is current
    double* d_carry = nullptr;          // [max_streams][2][ENC_STREAM_PCM_CARRY]
    long long* d_meta = nullptr;        // [max_batch + max_streams][ENC_SPCM_META]: a group's members, then the carry launch's entries
    size_t bytes = 0;
};

// frame `at` of the wire payload -> the mean of its C channels in double, as enc_pcm_kernel decodes it
static __device__ __forceinline__ double enc_spcm_frame(const void* __restrict__ raw, int is_f32, int C, size_t at) {
    double v = 0.0;
    if (is_f32) {
        const float* p = (const float*)raw + at * C;
        for (int c = 0; c < C; c++) v += (double)p[c];
    } else {
        const int16_t* p = (const int16_t*)raw + at * C;
        for (int c = 0; c < C; c++) v += (double)p[c] * (1.0 / 32768.0);
    }
    return v / (double)C;
}

// frame i of a stream that had n0 frames before this push and has n1 with it (its own zeros outside [0, n1)); cr: the carry row
// read, frames n0 - (J - 1) .. n0 - 1
static __device__ __forceinline__ double enc_spcm_at(long long i, long long n0, long long n1, int J, const double* __restrict__ cr,
                                                     const void* __restrict__ raw, int is_f32, int C, long long first) {
    if (i < 0 || i >= n1) return 0.0;
    if (i >= n0) return enc_spcm_frame(raw, is_f32, C, (size_t)(first + (i - n0)));
    const long long c = i - (n0 - (J - 1));
    return c >= 0 ? cr[c] : 0.0;   // (c < 0: further back than any output of this push reads)
}

__global__ void __launch_bounds__(ENC_SPCM_OUTPUTS) enc_stream_pcm_kernel(const void* __restrict__ raw, int is_f32, int C,
                                                                          const long long* __restrict__ meta,
                                                                          const double* __restrict__ taps,
                                                                          const double* __restrict__ carry, int up, int down,
                                                                          int half, int J, int W, float* __restrict__ y, int ld) {
    extern __shared__ __attribute__((aligned(16))) double spcm_sm[];
    double* st = spcm_sm;              // [J][up]
    double* xs = spcm_sm + J * up;     // [W] mono frames from i_first on
    const int tid = threadIdx.x, b = blockIdx.y;
    const long long* mt = meta + (size_t)b * ENC_SPCM_META;
    const long long first = mt[0], n0 = mt[1], n1 = mt[2], m_first = mt[3], n_out = mt[4];
    const double* cr = carry + (size_t)mt[5] * ENC_STREAM_PCM_CARRY;
    const int m0 = blockIdx.x * ENC_SPCM_OUTPUTS, ml = m0 + tid;
    if (m0 >= n_out) return;   // (the whole workgroup: no barrier is skipped by a part of it)
    for (int i = tid; i < J * up; i += ENC_SPCM_OUTPUTS) st[i] = taps[i];
    const long long i_first = ((m_first + m0) * down + half) / up - (J - 1);
    for (int k = tid; k < W; k += ENC_SPCM_OUTPUTS) xs[k] = enc_spcm_at(i_first + k, n0, n1, J, cr, raw, is_f32, C, first);
    __syncthreads();
    if (ml < n_out && ml < ld) {
        const long long a = (m_first + ml) * down + half, i0 = a / up;
        const int p = (int)(a - i0 * up);
        const double* xw = xs + (int)(i0 - i_first);   // in [J - 1, W - 1]: xw[-j] stays inside for j < J
        double acc = 0.0;
        for (int j = 0; j < J; j++) acc = fma(xw[-j], st[j * up + p], acc);
        y[(size_t)b * ld + ml] = (float)acc;
    }
}

// one workgroup per entry that brought frames: row written [k] = frame n1 - (J - 1) + k, k < J - 1
__global__ void __launch_bounds__(256) enc_stream_pcm_carry_kernel(const void* __restrict__ raw, int is_f32, int C,
                                                                   const long long* __restrict__ meta, double* carry, int J) {
    const long long* mt = meta + (size_t)blockIdx.x * ENC_SPCM_META;
    const long long first = mt[0], n0 = mt[1], n1 = mt[2];
    const double* cr = carry + (size_t)mt[5] * ENC_STREAM_PCM_CARRY;
    double* cw = carry + (size_t)mt[6] * ENC_STREAM_PCM_CARRY;
    for (int k = threadIdx.x; k < J - 1; k += 256) cw[k] = enc_spcm_at(n1 - (J - 1) + k, n0, n1, J, cr, raw, is_f32, C, first);
}

void enc_stream_pcm_release(EncStream* s) {
    if (!s || !s->pcm) return;
    if (s->pcm->d_carry) hipFree(s->pcm->d_carry);
    if (s->pcm->d_meta) hipFree(s->pcm->d_meta);
    delete s->pcm;
    s->pcm = nullptr;
}

namespace {

const char* const WHO = "enc_stream_push_pcm";

// the carry rows and the launch metadata, at the first push that gets this far
bool ensure_state(EncStream* s) {
    if (s->pcm) return true;
    EncStreamPcm* q = new EncStreamPcm;
    const size_t carry = sizeof(double) * (size_t)s->max_streams * 2 * ENC_STREAM_PCM_CARRY;
    const size_t meta = sizeof(long long) * ((size_t)s->e->max_batch + s->max_streams) * ENC_SPCM_META;
    if (hipMalloc((void**)&q->d_carry, carry) != hipSuccess || hipMalloc((void**)&q->d_meta, meta) != hipSuccess ||
        hipMemsetAsync(q->d_carry, 0, carry, s->e->s) != hipSuccess) {
        if (q->d_carry) hipFree(q->d_carry);
        if (q->d_meta) hipFree(q->d_meta);
        delete q;
        Q3_LOG("%s: no device memory for the carry rows of %d streams", WHO, s->max_streams);
        return false;
    }
    q->bytes = carry + meta;
    q->total_in.assign(s->max_streams, 0);
    q->format.assign(s->max_streams, 0);
    q->channels.assign(s->max_streams, 0);
    q->rate.assign(s->max_streams, 0);
    q->half.assign(s->max_streams, 0);
    s->pcm = q;
    return true;
}

// frames stream k has taken on its clip so far (a stream no enc_stream_push_pcm has fed since its reset is at 0)
long long frames_before(const EncStream* s, int k) { return s->pcm && s->source[k] == ENC_SRC_PCM ? s->pcm->total_in[k] : 0; }

// everything about a push but the samples' values and the capacity: the plan, and per entry the 24 kHz samples it hands on.
// Bad stream indices, streams named twice, finished streams and a clip enc_stream_push has fed are left to the plan of the walk.
bool check_push(const EncStream* s, int n, const int32_t* streams, int format, int channels, int rate, const int32_t* n_in,
                const int32_t* finish, EncPcmPlan* p, std::vector<int32_t>& n_new) {
    if (n < 0 || (n > 0 && (!streams || !n_in))) {
        Q3_LOG("%s: NULL streams or n_in", WHO);
        return false;
    }
    if (s->e->sample_rate != ENC_PCM_RATE) {
        Q3_LOG("%s: the front-end writes %d Hz, this encoder takes %d Hz", WHO, ENC_PCM_RATE, s->e->sample_rate);
        return false;
    }
    if (!enc_pcm_plan(format, channels, rate, p, WHO)) return false;
    const int most = enc_stream_pcm_max_frames_in(s->max_push, *p);
    n_new.assign(n, 0);
    for (int i = 0; i < n; i++) {
        const int k = streams[i];
        if (n_in[i] < 0 || n_in[i] > most) {
            Q3_LOG("%s: entry %d: %d input frames (0..%d at %d Hz: enc_stream_pcm_max_frames_in)", WHO, i, n_in[i], most, rate);
            return false;
        }
        if (k < 0 || k >= s->max_streams) continue;
        if (s->pcm && s->source[k] == ENC_SRC_PCM &&
            (s->pcm->format[k] != format || s->pcm->channels[k] != channels || s->pcm->rate[k] != rate)) {
            Q3_LOG("%s: stream %d began its clip as format %d, %d channels, %d Hz (enc_stream_reset starts the next clip)", WHO, k,
                   s->pcm->format[k], s->pcm->channels[k], s->pcm->rate[k]);
            return false;
        }
        n_new[i] = (int32_t)enc_stream_pcm_new(*p, frames_before(s, k), n_in[i], finish && finish[i]);
    }
    return true;
}

struct Feed : EncStreamFeed {
    EncStream* s = nullptr;
    EncPcmPlan p;
    int n = 0, format = 0, channels = 0;
    const int32_t *streams = nullptr, *n_in = nullptr;
    const void* pcm = nullptr;
    std::vector<long long> first;        // per entry: its first frame in the payload
    std::vector<long long> before;       // per entry: the frames its stream had taken
    long long frames = 0;
    bool uploaded = false;
    const double* taps = nullptr;
    float* samples_out = nullptr;        // the test hook's copy of the rows
    std::vector<long long> sample_off;   // per entry, into samples_out
    std::vector<std::vector<long long>> metas;   // (alive until the stream has drained: the uploads are asynchronous)

    void entry_meta(int en, long long* mt) const {
        const int k = streams[en];
        const long long n0 = before[en];
        const int cur = s->pcm->half[k];
        mt[0] = first[en];
        mt[1] = n0;
        mt[2] = n0 + n_in[en];
        mt[3] = enc_stream_pcm_ready(p, n0);
        mt[5] = 2 * k + cur;
        mt[6] = 2 * k + (cur ^ 1);
        mt[7] = 0;
    }
    int begin() override {
        Enc* e = s->e;
        if (!ensure_state(s)) return -1;
        taps = enc_pcm_table(e, p);
        if (!taps) return -1;
        const size_t bytes = (size_t)frames * channels * (format == ENC_PCM_F32 ? 4 : 2);
        if (!enc_pcm_raw_reserve(e, std::max<size_t>(bytes, 1), WHO)) return -1;
        const size_t lds = ((size_t)p.per_phase * p.up + (size_t)enc_pcm_window(p, ENC_SPCM_OUTPUTS)) * sizeof(double);
        if (lds > 48 * 1024)
            Q3_HIP(hipFuncSetAttribute((const void*)enc_stream_pcm_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), -1);
        return 0;
    }
    int upload() {   // the payload in its wire form, once, inside the push's timed span
        const size_t bytes = (size_t)frames * channels * (format == ENC_PCM_F32 ? 4 : 2);
        if (bytes && !uploaded) Q3_HIP(hipMemcpyAsync(s->e->pcm_raw, pcm, bytes, hipMemcpyHostToDevice, s->e->s), -1);
        uploaded = true;
        return 0;
    }
    int fill(const std::vector<int>& members, long long n_out) override {
        Enc* e = s->e;
        const int B = (int)members.size();
        if (upload()) return -1;
        metas.emplace_back((size_t)B * ENC_SPCM_META, 0);
        std::vector<long long>& meta = metas.back();
        for (int b = 0; b < B; b++) {
            entry_meta(members[b], &meta[(size_t)b * ENC_SPCM_META]);
            meta[(size_t)b * ENC_SPCM_META + 4] = n_out;
        }
        Q3_HIP(hipMemcpyAsync(s->pcm->d_meta, meta.data(), meta.size() * sizeof(long long), hipMemcpyHostToDevice, e->s), -1);
        const int W = (int)enc_pcm_window(p, ENC_SPCM_OUTPUTS);
        const size_t lds = ((size_t)p.per_phase * p.up + (size_t)W) * sizeof(double);
        const long ld = enc_pitch(s->max_push);
        hipLaunchKernelGGL(enc_stream_pcm_kernel, dim3((unsigned)((n_out + ENC_SPCM_OUTPUTS - 1) / ENC_SPCM_OUTPUTS), B),
                           dim3(ENC_SPCM_OUTPUTS), lds, e->s, (const void*)e->pcm_raw, format == ENC_PCM_F32 ? 1 : 0, channels,
                           (const long long*)s->pcm->d_meta, taps, (const double*)s->pcm->d_carry, p.up, p.down, p.half, p.per_phase, W,
                           s->d_pcm, (int)ld);
        Q3_HIP(hipGetLastError(), -1);
        if (samples_out)
            for (int b = 0; b < B; b++)
                Q3_HIP(hipMemcpyAsync(samples_out + sample_off[members[b]], s->d_pcm + (size_t)b * ld, sizeof(float) * (size_t)n_out,
                                      hipMemcpyDeviceToHost, e->s), -1);
        return 1;
    }
    int end() override {
        if (p.per_phase < 2) return 0;   // (24 kHz: nothing is carried)
        Enc* e = s->e;
        metas.emplace_back();
        std::vector<long long>& meta = metas.back();
        int B = 0;
        for (int en = 0; en < n; en++)
            if (n_in[en] > 0) {
                meta.resize((size_t)(B + 1) * ENC_SPCM_META, 0);
                entry_meta(en, &meta[(size_t)B * ENC_SPCM_META]);
                B++;
            }
        if (!B) return 0;
        if (upload()) return -1;
        long long* d = s->pcm->d_meta + (size_t)e->max_batch * ENC_SPCM_META;
        Q3_HIP(hipMemcpyAsync(d, meta.data(), meta.size() * sizeof(long long), hipMemcpyHostToDevice, e->s), -1);
        hipLaunchKernelGGL(enc_stream_pcm_carry_kernel, dim3(B), dim3(256), 0, e->s, (const void*)e->pcm_raw, format == ENC_PCM_F32 ? 1 : 0,
                           channels, (const long long*)d, s->pcm->d_carry, p.per_phase);
        Q3_HIP(hipGetLastError(), -1);
        return 1;
    }
};

int push_pcm(EncStream* s, int n, const int32_t* streams, const void* pcm, int format, int channels, int rate, const int32_t* n_in,
             const int32_t* finish, int64_t* codes_out, int64_t cap, int64_t* offsets, float* samples_out, int64_t* sample_offsets) {
    if (!s || !offsets) {
        Q3_LOG("%s: NULL object or offsets", WHO);
        return -1;
    }
    Feed f;   // (host work up to enc_stream_push_impl, which enters the handle)
    std::vector<int32_t> n_new;
    if (!check_push(s, n, streams, format, channels, rate, n_in, finish, &f.p, n_new)) return -1;
    f.first.assign(n, 0);
    f.before.assign(n, 0);
    f.sample_off.assign(n + 1, 0);
    for (int i = 0; i < n; i++) {
        const int k = streams[i];
        if (k >= 0 && k < s->max_streams) f.before[i] = frames_before(s, k);
        f.first[i] = f.frames;
        f.frames += n_in[i];
        f.sample_off[i + 1] = f.sample_off[i] + n_new[i];
    }
    const size_t samples = (size_t)f.frames * channels;
    if (samples > 0 && !pcm) {
        Q3_LOG("%s: NULL pcm", WHO);
        return -1;
    }
    if (format == ENC_PCM_F32) {
        const float* v = (const float*)pcm;
        for (size_t i = 0; i < samples; i++)
            if (!std::isfinite(v[i])) {
                Q3_LOG("%s: sample %zu is not finite", WHO, i);
                return -1;
            }
    }
    f.s = s;
    f.n = n;
    f.format = format;
    f.channels = channels;
    f.streams = streams;
    f.n_in = n_in;
    f.pcm = pcm;
    f.samples_out = samples_out;
    if (enc_stream_push_impl(s, n, streams, nullptr, n_new.data(), finish, codes_out, cap, offsets, nullptr, nullptr, &f)) return -1;
    EncStreamPcm* q = s->pcm;
    for (int i = 0; i < n; i++) {   // (the stream has drained: the rows the push wrote are the streams' carry now)
        const int k = streams[i];
        q->total_in[k] = f.before[i] + n_in[i];
        q->format[k] = format;
        q->channels[k] = channels;
        q->rate[k] = rate;
        if (f.p.per_phase > 1 && n_in[i] > 0) q->half[k] ^= 1;
    }
    if (sample_offsets) std::copy(f.sample_off.begin(), f.sample_off.end(), sample_offsets);
    return 0;
}

}  // namespace

}  // namespace q3

using namespace q3;

extern "C" {

int64_t enc_stream_pcm_samples(void* ss, int rate, int64_t n_in_total, int finished) {
    EncPcmPlan p;
    if (!ss || n_in_total < 0 || !enc_pcm_plan(ENC_PCM_S16, 1, rate, &p, "enc_stream_pcm_samples")) return -1;
    return (int64_t)enc_stream_pcm_total(p, n_in_total, finished != 0);
}

int enc_stream_pcm_max_frames_in(void* ss, int rate) {
    EncStream* s = (EncStream*)ss;
    EncPcmPlan p;
    if (!s || !enc_pcm_plan(ENC_PCM_S16, 1, rate, &p, "enc_stream_pcm_max_frames_in")) return -1;
    return q3::enc_stream_pcm_max_frames_in((long long)s->max_push, p);
}

int enc_stream_push_pcm_max_frames(void* ss, int n, const int32_t* streams, int format, int channels, int rate, const int32_t* n_in,
                                   const int32_t* finish) {
    EncStream* s = (EncStream*)ss;
    EncPcmPlan p;
    std::vector<int32_t> n_new;
    if (!s || !check_push(s, n, streams, format, channels, rate, n_in, finish, &p, n_new)) return -1;
    return enc_stream_plan_frames(s, n, streams, n_new.data(), finish, ENC_SRC_PCM);
}

int enc_stream_push_pcm(void* s, int n, const int32_t* streams, const void* pcm, int format, int channels, int rate,
                        const int32_t* n_in, const int32_t* finish, int64_t* codes_out, int64_t out_capacity_frames, int64_t* offsets) {
    return push_pcm((EncStream*)s, n, streams, pcm, format, channels, rate, n_in, finish, codes_out, out_capacity_frames, offsets, nullptr,
                    nullptr);
}

int64_t enc_stream_pcm_device_bytes(void* ss) {
    EncStream* s = (EncStream*)ss;
    return !s ? -1 : s->pcm ? (int64_t)s->pcm->bytes : 0;
}

// test hook (not in the header, beside enc_debug_pcm): the same push, and per entry the 24 kHz f32 samples it handed to the op
// table: entry i's are samples_out[sample_offsets[i] .. sample_offsets[i + 1]) (sample_offsets [n + 1]; the caller sizes
// samples_out for n entries of max_push_samples)
int enc_stream_debug_push_pcm(void* s, int n, const int32_t* streams, const void* pcm, int format, int channels, int rate,
                              const int32_t* n_in, const int32_t* finish, int64_t* codes_out, int64_t out_capacity_frames,
                              int64_t* offsets, float* samples_out, int64_t* sample_offsets) {
    if (!samples_out || !sample_offsets) return -1;
    return push_pcm((EncStream*)s, n, streams, pcm, format, channels, rate, n_in, finish, codes_out, out_capacity_frames, offsets,
                    samples_out, sample_offsets);
}

}  // extern "C"
