// q3_enc_pcm_host.h -- the host arithmetic of the encoder's PCM front-end (csrc/q3_enc_pcm.hip, enc_encode_pcm): the rules
// of scipy.signal.resample_poly with its defaults, in double.  Plain C++, no HIP and no other header of the library: a CPU
// driver compiles it alone (tests/pcm_host_driver.cpp, also under ASan/UBSan).
//
//   g = gcd(rate, 24000), up = 24000 / g, down = rate / g; up == down == 1: no filter (the one tap 1.0)
//   mr = max(up, down), half = 10 mr, N = 2 half + 1
//   h[k] = up w[k] / sum(w),  w[k] = (1 / mr) sinc((k - half) / mr) I0(5 sqrt(1 - ((k - half) / half)^2)) / I0(5)
//        (= up * firwin(N, 1 / mr, window=("kaiser", 5.0)))
//   n_out = ceil(n up / down),  y[m] = sum_i x[i] h[m down + half - i up] over 0 <= i < n with the tap index in [0, N)
//
// The device reads the taps by phase: output m uses h[p + j up], j = 0 .. per_phase - 1, p = (m down + half) mod up, against
// x[i0 - j], i0 = (m down + half) / up.  enc_pcm_polyphase lays them out [j][p] (zero where p + j up >= N).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace q3 {

constexpr int ENC_PCM_RATE = 24000;        // what the front-end writes
constexpr int ENC_PCM_MAX_CHANNELS = 8;
constexpr int ENC_PCM_MIN_RATE = 8000, ENC_PCM_MAX_RATE = 192000;
constexpr int ENC_PCM_MAX_FACTOR = 640;    // max(up, down): the table stays at or below 12 801 doubles

#define Q3_PCM_LOG(...)                             \
    do {                                            \
        fprintf(stderr, "[qwen3tts] " __VA_ARGS__); \
        fputc('\n', stderr);                        \
    } while (0)

struct EncPcmPlan {
    int up = 1, down = 1;
    int half = 0, n_taps = 1;   // N = 2 half + 1 (no filter: the one tap 1.0 at index 0)
    int per_phase = 1;          // ceil(N / up): the terms of one output at most
};

static inline int enc_pcm_gcd(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// reduced factors -> the filter's geometry; false: a factor outside 1..ENC_PCM_MAX_FACTOR
static inline bool enc_pcm_plan_factors(int up, int down, EncPcmPlan* p) {
    const int mr = up > down ? up : down;
    if (up < 1 || down < 1 || mr > ENC_PCM_MAX_FACTOR) return false;
    EncPcmPlan q;
    q.up = up;
    q.down = down;
    if (mr > 1) {
        q.half = 10 * mr;
        q.n_taps = 2 * q.half + 1;
    }
    q.per_phase = (q.n_taps + q.up - 1) / q.up;
    *p = q;
    return true;
}

// format (0: s16le, 1: f32le), channels and rate of a call -> the plan, or false with one logged line
static inline bool enc_pcm_plan(int format, int channels, int rate, EncPcmPlan* p, const char* who) {
    if (format != 0 && format != 1) {
        Q3_PCM_LOG("%s: format %d is neither ENC_PCM_S16 (0) nor ENC_PCM_F32 (1)", who, format);
        return false;
    }
    if (channels < 1 || channels > ENC_PCM_MAX_CHANNELS) {
        Q3_PCM_LOG("%s: %d channels (1..%d)", who, channels, ENC_PCM_MAX_CHANNELS);
        return false;
    }
    if (rate < ENC_PCM_MIN_RATE || rate > ENC_PCM_MAX_RATE) {
        Q3_PCM_LOG("%s: rate %d Hz outside %d..%d", who, rate, ENC_PCM_MIN_RATE, ENC_PCM_MAX_RATE);
        return false;
    }
    const int g = enc_pcm_gcd(rate, ENC_PCM_RATE);
    if (!enc_pcm_plan_factors(ENC_PCM_RATE / g, rate / g, p)) {
        Q3_PCM_LOG("%s: rate %d Hz resamples by %d/%d, a factor above %d", who, rate, ENC_PCM_RATE / g, rate / g, ENC_PCM_MAX_FACTOR);
        return false;
    }
    return true;
}

// ceil(n_in up / down) in 64 bits (n_in up to 2^31 - 1 times 640 stays far inside)
static inline long long enc_pcm_out_len(const EncPcmPlan& p, long long n_in) {
    return n_in <= 0 ? 0 : (n_in * (long long)p.up + p.down - 1) / p.down;
}

// a clip of n_in frames -> its output length in 1..max_samples, or -1 with one logged line
static inline int enc_pcm_clip_out(const EncPcmPlan& p, long long n_in, int max_samples, const char* who, int clip) {
    if (n_in <= 0 || n_in > 0x7fffffffLL) {
        Q3_PCM_LOG("%s: clip %d has %lld input frames (at least 1)", who, clip, n_in);
        return -1;
    }
    const long long n_out = enc_pcm_out_len(p, n_in);
    if (n_out < 1 || n_out > (long long)max_samples) {
        Q3_PCM_LOG("%s: clip %d gives %lld samples at %d Hz (1..%d)", who, clip, n_out, ENC_PCM_RATE, max_samples);
        return -1;
    }
    return (int)n_out;
}

// modified Bessel function of the first kind, order 0: sum_k ((x / 2)^k / k!)^2, terms until they stop changing the sum
static inline double enc_pcm_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; k++) {
        term *= q / ((double)k * (double)k);
        const double next = sum + term;
        if (next == sum) break;
        sum = next;
    }
    return sum;
}

// the N taps h[k], in double
static inline void enc_pcm_taps(const EncPcmPlan& p, std::vector<double>& h) {
    h.assign((size_t)p.n_taps, 1.0);
    if (p.n_taps == 1) return;
    const double pi = 3.14159265358979323846;
    const int mr = p.up > p.down ? p.up : p.down;
    const double i0b = enc_pcm_i0(5.0);
    double sum = 0.0, lost = 0.0;   // (the sum compensated: its order is no freedom of the design)
    for (int k = 0; k < p.n_taps; k++) {
        const double m = (double)(k - p.half);
        const double a = m / (double)mr, r = m / (double)p.half;
        const double sinc = k == p.half ? 1.0 : std::sin(pi * a) / (pi * a);
        double in = 1.0 - r * r;
        if (in < 0.0) in = 0.0;
        h[(size_t)k] = (1.0 / (double)mr) * sinc * (enc_pcm_i0(5.0 * std::sqrt(in)) / i0b);
        const double v = h[(size_t)k], t = sum + v;
        lost += std::fabs(sum) >= std::fabs(v) ? (sum - t) + v : (v - t) + sum;
        sum = t;
    }
    sum += lost;
    for (int k = 0; k < p.n_taps; k++) h[(size_t)k] = (double)p.up * h[(size_t)k] / sum;
}

// taps by phase for the device, [per_phase][up]: t[j * up + ph] = h[ph + j * up], 0 past the last tap
static inline void enc_pcm_polyphase(const EncPcmPlan& p, const std::vector<double>& h, std::vector<double>& t) {
    t.assign((size_t)p.per_phase * p.up, 0.0);
    for (int k = 0; k < p.n_taps; k++) t[(size_t)(k / p.up) * p.up + (size_t)(k % p.up)] = h[(size_t)k];
}

// input frames one workgroup of `outputs` consecutive outputs can touch: i0 moves by at most outputs * down / up + 1 across
// them, and every output reaches per_phase - 1 frames back
static inline long long enc_pcm_window(const EncPcmPlan& p, int outputs) {
    return ((long long)(outputs - 1) * p.down) / p.up + 1 + p.per_phase;
}

}  // namespace q3
