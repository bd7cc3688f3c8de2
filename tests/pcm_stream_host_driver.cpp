// pcm_stream_host_driver.cpp -- the host arithmetic of the streaming encode's PCM front-end (csrc/q3_enc_stream_pcm_host.h over
// csrc/q3_enc_pcm_host.h) as a stand-alone program, for tests/test_enc_stream_pcm_contract.py.  The two headers are plain C++:
// no device header, no library.  Built plain and with -fsanitize=address,undefined and run on the CPU.
//
//   pcm_stream_host_driver [step]
//
// For every reduced (up, down) a rate of 8000..192000 Hz gives with both factors <= 640 (step > 1: every step-th of them and
// the listed rates) it walks a carry-state resample in double -- the stream's rule: ready(n) outputs after n frames, the last
// J - 1 frames carried -- over several splits of one clip and requires
//   - the samples handed out after every push to be ready(n), and ceil(n up / down) after the finish,
//   - the joined output to be bit-equal to the whole-clip sum of q3_enc_pcm_host.h's rule,
//   - a push of max_frames_in frames to fit max_push at every phase, finishing or not, for max_push in {32, 1920, 24000},
//   - max_frames_in >= floor((max_push - 32) down / up), and the carry to stay within ENC_STREAM_PCM_CARRY.
// Prints "ok <pairs> <pushes>" and exits 0, or the first failures and exits 1.
#include "../qwen3_tts_axera_russian_amd/csrc/q3_enc_stream_pcm_host.h"

#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>

using namespace q3;

static unsigned long long rng_state = 0x9e3779b97f4a7c15ULL;
static unsigned rnd() {
    rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL;
    return (unsigned)(rng_state >> 33);
}

static int failures = 0;
#define FAIL(...)                     \
    do {                              \
        if (failures++ < 20) {        \
            fprintf(stderr, __VA_ARGS__); \
            fputc('\n', stderr);      \
        }                             \
    } while (0)

// the whole-clip rule: y[m] = sum_j x[i0 - j] t[j][p], frames outside [0, n) zero
static void whole(const EncPcmPlan& p, const std::vector<double>& t, const std::vector<double>& x, std::vector<double>& y) {
    const long long n = (long long)x.size();
    y.assign((size_t)enc_pcm_out_len(p, n), 0.0);
    for (long long m = 0; m < (long long)y.size(); m++) {
        const long long a = m * p.down + p.half, i0 = a / p.up;
        const int ph = (int)(a - i0 * p.up);
        double acc = 0.0;
        for (int j = 0; j < p.per_phase; j++) {
            const long long i = i0 - j;
            acc = std::fma(i >= 0 && i < n ? x[(size_t)i] : 0.0, t[(size_t)j * p.up + ph], acc);
        }
        y[(size_t)m] = acc;
    }
}

struct Stream {
    const EncPcmPlan& p;
    const std::vector<double>& t;
    std::vector<double> carry;   // frames n0 - (J - 1) .. n0 - 1
    long long n0 = 0;
    std::vector<double> out;
    Stream(const EncPcmPlan& p_, const std::vector<double>& t_) : p(p_), t(t_), carry((size_t)(p_.per_phase - 1), 0.0) {}
    // -> samples handed out by this push
    long long push(const double* x, long long k, bool fin) {
        const int J = p.per_phase;
        const long long n1 = n0 + k, m_first = enc_stream_pcm_ready(p, n0), m_end = enc_stream_pcm_total(p, n1, fin);
        auto at = [&](long long i) -> double {
            if (i < 0 || i >= n1) return 0.0;
            if (i >= n0) return x[i - n0];
            const long long c = i - (n0 - (J - 1));
            if (c < 0) {
                FAIL("up %d down %d: a push from %lld frames reads frame %lld, behind the carry", p.up, p.down, n0, i);
                return 0.0;
            }
            return carry[(size_t)c];
        };
        for (long long m = m_first; m < m_end; m++) {
            const long long a = m * p.down + p.half, i0 = a / p.up;
            const int ph = (int)(a - i0 * p.up);
            if (!fin && i0 > n1 - 1) FAIL("up %d down %d: output %lld is handed out before its frame %lld", p.up, p.down, m, i0);
            double acc = 0.0;
            for (int j = 0; j < J; j++) acc = std::fma(at(i0 - j), t[(size_t)j * p.up + ph], acc);
            out.push_back(acc);
        }
        std::vector<double> next((size_t)(J - 1), 0.0);
        for (int c = 0; c < J - 1; c++) next[(size_t)c] = at(n1 - (J - 1) + c);
        carry.swap(next);
        n0 = n1;
        if (enc_stream_pcm_new(p, n1 - k, k, fin) != m_end - m_first) FAIL("up %d down %d: enc_stream_pcm_new disagrees", p.up, p.down);
        return m_end - m_first;
    }
};

static long long pushes = 0;

// kind 0: one finishing push; 1: one frame at a time, then a finish with 0 frames; 2: pushes shorter than J - 1 with 0-frame
// pushes between them; 3: random cuts; 4: 1 / 2 / 3 frames; 5: every 7th frame
static void run_split(const EncPcmPlan& p, const std::vector<double>& t, const std::vector<double>& x, const std::vector<double>& want,
                      int kind) {
    Stream s(p, t);
    const long long n = (long long)x.size();
    const int J = p.per_phase;
    long long at = 0, handed = 0;
    int step = 0;
    bool done = false;
    while (!done) {
        long long k;
        bool fin = false;
        switch (kind) {
            case 0: k = n; fin = true; break;
            case 1: k = at < n ? 1 : 0; fin = at >= n; break;
            case 2: k = (step % 3 == 1) ? 0 : (J > 2 ? 1 + rnd() % (unsigned)(J - 2) : 1); break;
            case 3: k = rnd() % (unsigned)(4 * J + 5); break;
            case 4: k = 1 + step % 3; break;
            default: k = 7; break;
        }
        if (kind >= 2) {
            if (k >= n - at) {
                k = n - at;
                fin = (rnd() & 1) || kind == 5;   // the last frames and the finish together, or ...
            }
            if (at == n && k == 0 && step > 0 && !fin) fin = true;   // ... a finish with 0 new frames
        }
        handed += s.push(x.data() + at, k, fin);
        at += k;
        pushes++;
        step++;
        const long long rule = fin ? enc_pcm_out_len(p, at) : enc_stream_pcm_ready(p, at);
        if (handed != rule || handed != (long long)s.out.size())
            FAIL("up %d down %d split %d: %lld samples after %lld frames (finish %d), the rule says %lld", p.up, p.down, kind, handed, at,
                 (int)fin, rule);
        done = fin;
    }
    if (at != n) FAIL("up %d down %d split %d: the walk stopped at %lld of %lld frames", p.up, p.down, kind, at, n);
    if (s.out.size() != want.size() || (want.size() && memcmp(s.out.data(), want.data(), want.size() * sizeof(double))))
        FAIL("up %d down %d split %d: the joined output is not the whole clip's, bit for bit", p.up, p.down, kind);
}

static void run_pair(int up, int down) {
    EncPcmPlan p;
    if (!enc_pcm_plan_factors(up, down, &p)) {
        FAIL("up %d down %d refused", up, down);
        return;
    }
    const int J = p.per_phase;
    if (J - 1 > ENC_STREAM_PCM_CARRY) FAIL("up %d down %d: carries %d frames, above %d", up, down, J - 1, ENC_STREAM_PCM_CARRY);
    if (up == 1 && down == 1 && (J != 1 || enc_stream_pcm_ready(p, 5) != 5)) FAIL("24 kHz: J %d, ready(5) %lld", J, enc_stream_pcm_ready(p, 5));
    std::vector<double> h, t;
    enc_pcm_taps(p, h);
    enc_pcm_polyphase(p, h, t);
    // clips: 0 and 1 frames, and one of a few J with a ragged end
    const long long lens[3] = {0, 1, 3LL * J + 2 + (long long)(rnd() % (unsigned)(2 * down + 3))};
    for (long long n : lens) {
        std::vector<double> x((size_t)n), want;
        for (auto& v : x) v = ((double)rnd() / 2147483648.0 - 1.0) * (rnd() % 5 == 0 ? 1e-3 : 1.0);
        whole(p, t, x, want);
        if (n == 0 && !want.empty()) FAIL("up %d down %d: 0 frames give samples", up, down);
        for (int kind = 0; kind < 6; kind++) run_split(p, t, x, want, kind);
        // the tail a finish hands out beyond ready(n)
        const long long tail = enc_pcm_out_len(p, n) - enc_stream_pcm_ready(p, n);
        if (tail < 0 || tail > 31) FAIL("up %d down %d: the finish of %lld frames hands out %lld samples", up, down, n, tail);
    }
    for (long long max_push : {32LL, 1920LL, 24000LL}) {
        const long long k = enc_stream_pcm_max_frames_in(max_push, p);
        const long long floor_ = (max_push - 32) * down / up;
        if (k < floor_ || k < 0) FAIL("up %d down %d max_push %lld: max_frames_in %lld below %lld", up, down, max_push, k, floor_);
        const long long phases = 2LL * down + (p.half + up) / up + 2;
        for (long long n0 = 0; n0 <= phases; n0++)
            for (int fin = 0; fin < 2; fin++) {
                const long long got = enc_stream_pcm_new(p, n0, k, fin != 0);
                if (got > max_push || got < 0)
                    FAIL("up %d down %d max_push %lld: %lld frames after %lld (finish %d) give %lld samples", up, down, max_push, k, n0, fin, got);
            }
    }
}

int main(int argc, char** argv) {
    const int step = argc > 1 ? atoi(argv[1]) : 1;
    if (step < 1) return 2;
    const int listed[] = {8000, 8120, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 184000, 192000};
    std::set<std::pair<int, int>> pairs;
    int seen = 0;
    for (int rate = ENC_PCM_MIN_RATE; rate <= ENC_PCM_MAX_RATE; rate++) {
        const int g = enc_pcm_gcd(rate, ENC_PCM_RATE), up = ENC_PCM_RATE / g, down = rate / g;
        if (up > ENC_PCM_MAX_FACTOR || down > ENC_PCM_MAX_FACTOR) continue;
        bool take = seen++ % step == 0;
        for (int r : listed) take = take || r == rate;
        if (take) pairs.insert({up, down});
    }
    for (int r : listed) {
        const int g = enc_pcm_gcd(r, ENC_PCM_RATE);
        if (!pairs.count({ENC_PCM_RATE / g, r / g})) FAIL("rate %d is not covered", r);
    }
    for (const auto& pr : pairs) run_pair(pr.first, pr.second);
    if (failures) {
        fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    printf("ok %zu %lld\n", pairs.size(), pushes);
    return 0;
}
