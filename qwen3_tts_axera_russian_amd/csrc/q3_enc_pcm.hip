// q3_enc_pcm.hip -- the encoder's PCM front-end for gfx950 (enc_encode_pcm, include/qwen3tts_enc_pcm.h): interleaved s16le / f32le
// PCM of 1..8 channels at a client's rate -> 24 kHz mono f32 in the handle's pcm rows, which enc_run then encodes as if
// enc_encode had uploaded them.  The arithmetic is q3_enc_pcm_host.h's (scipy.signal.resample_poly's rules): taps designed on
// the host in double, every output a float64 sum rounded once to float32.
//
// enc_pcm_kernel, one launch per call for all B clips (grid: 256 outputs x clip).  A workgroup's 256 consecutive outputs of one
// clip read one window of input frames -- i0(m) = (m down + half) / up moves by at most 255 down / up + 1 across them and
// every output reaches per_phase - 1 frames back -- which the workgroup reads once, lanes on consecutive frames (the
// interleaved payload in its wire form, coalesced), decodes, downmixes in double and keeps in LDS with zeros for the frames
// before 0 and from n_in on: the inner loop has no bounds check.  The tap table [per_phase][up] (at most ~13 000 doubles) is
// copied to LDS linearly; output m reads phase p = (m down + half) mod up of row j against window frame i0 - j.  Within one
// row the lanes' phases step by down mod up (coprime to up: distinct while up >= 64, broadcasts below), so both operands of
// the sum come from LDS whatever the rate.  Outputs at or past a clip's n_out, up to the row pitch, are written 0: the rows are
// as enc_upload leaves them.
#include "../../include/qwen3tts_enc.h"
#include "q3_enc.h"
#include "q3_enc_pcm_host.h"

#include <algorithm>
#include <cmath>

namespace q3 {

constexpr int ENC_PCM_OUTPUTS = 256;   // per workgroup, one per thread
constexpr int ENC_PCM_TABLES = 4;      // tap tables a handle keeps

__global__ void __launch_bounds__(ENC_PCM_OUTPUTS) enc_pcm_kernel(const void* __restrict__ raw, int is_f32, int C,
                                                                  const long long* __restrict__ meta,
                                                                  const double* __restrict__ taps, int up, int down, int half,
                                                                  int J, int W, float* __restrict__ y, int ld) {
    extern __shared__ __attribute__((aligned(16))) double pcm_sm[];
    double* st = pcm_sm;              // [J][up]
    double* xs = pcm_sm + J * up;     // [W] mono frames from i_first on
    const int tid = threadIdx.x, b = blockIdx.y;
    const int m0 = blockIdx.x * ENC_PCM_OUTPUTS, m = m0 + tid;
    const long long first = meta[3 * b], n_in = meta[3 * b + 1], n_out = meta[3 * b + 2];
    float* yb = y + (size_t)b * ld;
    if (m0 >= n_out) {   // (the whole workgroup: no barrier is skipped by a part of it)
        if (m < ld) yb[m] = 0.f;
        return;
    }
    for (int i = tid; i < J * up; i += ENC_PCM_OUTPUTS) st[i] = taps[i];
    const long long i_first = ((long long)m0 * down + half) / up - (J - 1);
    for (int k = tid; k < W; k += ENC_PCM_OUTPUTS) {
        const long long i = i_first + k;
        double v = 0.0;
        if (i >= 0 && i < n_in) {
            const size_t at = (size_t)(first + i) * C;
            if (is_f32) {
                const float* p = (const float*)raw + at;
                for (int c = 0; c < C; c++) v += (double)p[c];
            } else {
                const int16_t* p = (const int16_t*)raw + at;
                for (int c = 0; c < C; c++) v += (double)p[c] * (1.0 / 32768.0);
            }
            v = v / (double)C;
        }
        xs[k] = v;
    }
    __syncthreads();
    if (m < ld) {
        float out = 0.f;
        if (m < n_out) {
            const long long a = (long long)m * down + half, i0 = a / up;
            const int p = (int)(a - i0 * up);
            const double* xw = xs + (int)(i0 - i_first);   // in [J - 1, W - 1]: xw[-j] stays inside for j < J
            double acc = 0.0;
            for (int j = 0; j < J; j++) acc = fma(xw[-j], st[j * up + p], acc);
            out = (float)acc;
        }
        yb[m] = out;
    }
}

void enc_pcm_release(Enc* e) {
    for (auto& t : e->pcm_tables)
        if (t.taps) hipFree(t.taps);
    e->pcm_tables.clear();
    if (e->pcm_raw) hipFree(e->pcm_raw);
    if (e->pcm_meta) hipFree(e->pcm_meta);
    e->pcm_raw = nullptr;
    e->pcm_meta = nullptr;
    e->pcm_raw_bytes = 0;
}

// the device table of the plan: one the handle kept, or built now in place of the least recently used of ENC_PCM_TABLES
const double* enc_pcm_table(Enc* e, const EncPcmPlan& p) {
    e->pcm_calls++;
    for (auto& t : e->pcm_tables)
        if (t.up == p.up && t.down == p.down) {
            t.used = e->pcm_calls;
            return t.taps;
        }
    std::vector<double> h, poly;
    enc_pcm_taps(p, h);
    enc_pcm_polyphase(p, h, poly);
    double* d = nullptr;
    if (hipMalloc((void**)&d, poly.size() * sizeof(double)) != hipSuccess ||
        hipMemcpy(d, poly.data(), poly.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
        if (d) hipFree(d);
        Q3_LOG("enc_encode_pcm: no device memory for a tap table of %zu doubles", poly.size());
        return nullptr;
    }
    if ((int)e->pcm_tables.size() >= ENC_PCM_TABLES) {   // (every call drains the stream before it returns: nothing reads it)
        auto old = std::min_element(e->pcm_tables.begin(), e->pcm_tables.end(),
                                    [](const Enc::PcmTable& x, const Enc::PcmTable& y) { return x.used < y.used; });
        hipFree(old->taps);
        e->pcm_tables.erase(old);
    }
    Enc::PcmTable t;
    t.up = p.up;
    t.down = p.down;
    t.taps = d;
    t.used = e->pcm_calls;
    e->pcm_tables.push_back(t);
    return d;
}

bool enc_pcm_raw_reserve(Enc* e, size_t bytes, const char* who) {
    if (bytes <= e->pcm_raw_bytes) return true;
    // grows to the largest payload seen (at most 8 channels x 8 input frames per sample)
    if (e->pcm_raw) hipFree(e->pcm_raw);
    e->pcm_raw = nullptr;
    e->pcm_raw_bytes = 0;
    if (hipMalloc(&e->pcm_raw, bytes) != hipSuccess) {
        Q3_LOG("%s: no device memory for a payload of %zu bytes", who, bytes);
        return false;
    }
    e->pcm_raw_bytes = bytes;
    return true;
}

// checks the call, uploads the payload in its wire form and launches the front-end -> lens = the clips' 24 kHz lengths; 0 / <0
static int enc_pcm_prepare(Enc* e, const void* pcm, int format, int channels, int rate, const int32_t* n_in, int B,
                           std::vector<int>& lens, const char* who) {
    if (!pcm || !n_in) {
        Q3_LOG("%s: NULL pcm or n_in", who);
        return -1;
    }
    if (B < 1 || B > e->max_batch) {
        Q3_LOG("%s: B = %d outside 1..%d (max_batch)", who, B, e->max_batch);
        return -1;
    }
    if (e->sample_rate != ENC_PCM_RATE) {
        Q3_LOG("%s: the front-end writes %d Hz, this encoder takes %d Hz", who, ENC_PCM_RATE, e->sample_rate);
        return -1;
    }
    EncPcmPlan p;
    if (!enc_pcm_plan(format, channels, rate, &p, who)) return -1;
    lens.assign(e->max_batch, 0);
    std::vector<long long>& meta = e->pcm_meta_host;
    meta.assign((size_t)e->max_batch * 3, 0);
    long long frames = 0;
    for (int b = 0; b < B; b++) {
        const int n_out = enc_pcm_clip_out(p, n_in[b], e->max_samples, who, b);
        if (n_out < 0) return -1;
        lens[b] = n_out;
        meta[3 * b] = frames;
        meta[3 * b + 1] = n_in[b];
        meta[3 * b + 2] = n_out;
        frames += n_in[b];
    }
    const size_t samples = (size_t)frames * channels, bytes = samples * (format == ENC_PCM_F32 ? 4 : 2);
    if (format == ENC_PCM_F32) {
        const float* f = (const float*)pcm;
        for (size_t i = 0; i < samples; i++)
            if (!std::isfinite(f[i])) {
                Q3_LOG("%s: sample %zu is not finite", who, i);
                return -1;
            }
    }
    const double* taps = enc_pcm_table(e, p);
    if (!taps) return -1;
    if (!e->pcm_meta) Q3_HIP(hipMalloc((void**)&e->pcm_meta, (size_t)e->max_batch * 3 * sizeof(long long)), -1);
    if (!enc_pcm_raw_reserve(e, bytes, who)) return -1;
    const long L = *std::max_element(lens.begin(), lens.begin() + B), ld = enc_pitch(L);
    const int W = (int)enc_pcm_window(p, ENC_PCM_OUTPUTS);
    const size_t lds = ((size_t)p.per_phase * p.up + (size_t)W) * sizeof(double);
    if (lds > 48 * 1024)
        Q3_HIP(hipFuncSetAttribute((const void*)enc_pcm_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), -1);
    Q3_HIP(hipMemcpyAsync(e->pcm_raw, pcm, bytes, hipMemcpyHostToDevice, e->s), -1);
    Q3_HIP(hipMemcpyAsync(e->pcm_meta, meta.data(), meta.size() * sizeof(long long), hipMemcpyHostToDevice, e->s), -1);
    hipLaunchKernelGGL(enc_pcm_kernel, dim3((unsigned)(ld / ENC_PCM_OUTPUTS + (ld % ENC_PCM_OUTPUTS ? 1 : 0)), B),
                       dim3(ENC_PCM_OUTPUTS), lds, e->s, (const void*)e->pcm_raw, format == ENC_PCM_F32 ? 1 : 0, channels,
                       (const long long*)e->pcm_meta, taps, p.up, p.down, p.half, p.per_phase, W, e->pcm, (int)ld);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

}  // namespace q3

using namespace q3;

extern "C" {

int enc_pcm_frames(void* h, int n_in, int rate) {
    Enc* e = (Enc*)h;
    if (!e) return -1;
    EncPcmPlan p;
    if (!enc_pcm_plan(ENC_PCM_S16, 1, rate, &p, "enc_pcm_frames")) return -1;
    const int n_out = enc_pcm_clip_out(p, n_in, e->max_samples, "enc_pcm_frames", 0);
    return n_out < 0 ? -1 : enc_frames(e, n_out);
}

int enc_encode_pcm(void* h, const void* pcm, int format, int channels, int rate, const int32_t* n_in, int B, int64_t* codes_out,
                   int max_frames, int32_t* n_frames) {
    Enc* e = (Enc*)h;
    if (!e) {
        Q3_LOG("enc_encode_pcm: NULL handle");
        return -1;
    }
    enc_enter(e);
    if (!codes_out || !n_frames) {
        Q3_LOG("enc_encode_pcm: NULL codes_out or n_frames");
        return -1;
    }
    std::vector<int> lens;
    Q3_HIP(hipEventRecord(e->e0, e->s), -1);
    if (enc_pcm_prepare(e, pcm, format, channels, rate, n_in, B, lens, "enc_encode_pcm")) return -1;
    for (int b = 0; b < B; b++) {
        const int f = enc_frames(e, lens[b]);
        if (f > max_frames) {   // (the launch above only wrote the handle's own rows)
            Q3_LOG("enc_encode_pcm: clip %d gives %d frames, codes_out holds %d per clip", b, f, max_frames);
            hipStreamSynchronize(e->s);
            return -1;
        }
    }
    float* out = nullptr;
    int C = 0;
    long T = 0;
    if (enc_run(e, B, lens, -1, &out, &C, &T)) return -1;
    return enc_collect_codes(e, B, lens, T, codes_out, max_frames, n_frames);
}

int enc_resample_pcm(void* h, const void* pcm, int format, int channels, int rate, const int32_t* n_in, int B, float* out, int out_pitch,
                     int32_t* n_out) {
    Enc* e = (Enc*)h;
    if (!e) {
        Q3_LOG("enc_resample_pcm: NULL handle");
        return -1;
    }
    enc_enter(e);
    if (!out || !n_out) {
        Q3_LOG("enc_resample_pcm: NULL out or n_out");
        return -1;
    }
    std::vector<int> lens;
    if (enc_pcm_prepare(e, pcm, format, channels, rate, n_in, B, lens, "enc_resample_pcm")) return -1;
    for (int b = 0; b < B; b++)
        if (lens[b] > out_pitch) {   // (the launch above only wrote the handle's own rows)
            Q3_LOG("enc_resample_pcm: clip %d gives %d samples, out holds %d per clip", b, lens[b], out_pitch);
            hipStreamSynchronize(e->s);
            return -1;
        }
    const long pitch = enc_pitch(*std::max_element(lens.begin(), lens.begin() + B));
    for (int b = 0; b < B; b++)
        Q3_HIP(hipMemcpyAsync(out + (size_t)b * out_pitch, e->pcm + (size_t)b * pitch, (size_t)lens[b] * sizeof(float), hipMemcpyDeviceToHost,
                              e->s), -1);
    Q3_HIP(hipStreamSynchronize(e->s), -1);
    for (int b = 0; b < B; b++) n_out[b] = lens[b];
    return 0;
}

// test hook (not in the header, beside enc_debug_run): the rows the front-end prepares, whole pitch rows so that the zeros past
// a clip's length can be seen: out [B][*ld] f32, *ld = the longest clip's 24 kHz length rounded up to 32 (the caller sizes out
// for that: the lengths follow from n_in and the rate), n_out[B] the clips' lengths
int enc_debug_pcm(void* h, const void* pcm, int format, int channels, int rate, const int32_t* n_in, int B, float* out,
                  int32_t* n_out, int* ld) {
    Enc* e = (Enc*)h;
    if (!e || !out || !n_out || !ld) return -1;
    enc_enter(e);
    std::vector<int> lens;
    if (enc_pcm_prepare(e, pcm, format, channels, rate, n_in, B, lens, "enc_debug_pcm")) return -1;
    const long pitch = enc_pitch(*std::max_element(lens.begin(), lens.begin() + B));
    Q3_HIP(hipMemcpyAsync(out, e->pcm, (size_t)B * pitch * sizeof(float), hipMemcpyDeviceToHost, e->s), -1);
    Q3_HIP(hipStreamSynchronize(e->s), -1);
    for (int b = 0; b < B; b++) n_out[b] = lens[b];
    *ld = (int)pitch;
    return 0;
}

}  // extern "C"
