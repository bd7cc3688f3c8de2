// q3_enc_stream_pcm_host.h -- the host arithmetic of the streaming encode's PCM front-end (csrc/q3_enc_stream_pcm.hip,
// enc_stream_push_pcm): which 24 kHz samples a stream's input frames have settled, what it carries between pushes and how
// many input frames one push may bring.  Plain C++ over q3_enc_pcm_host.h, no device header and no other header of the library:
// a CPU driver compiles the two alone (tests/pcm_stream_host_driver.cpp, also under ASan/UBSan).
//
// With up, down, half and J = per_phase of the plan, output m of the whole-clip rule reads frames i0(m) - j, j < J,
// i0(m) = (m down + half) / up, frames outside the clip as zeros.  After n frames of an unfinished stream the outputs whose
// newest frame has arrived, i0(m) <= n - 1, are final -- that is m down + half <= n up - 1:
//
//   ready(n) = n up - 1 - half < 0 ? 0 : (n up - 1 - half) / down + 1        (at 24 kHz: n)
//
// and the finish brings the total to ceil(n up / down), the frames from n on read as the zeros the whole-clip kernel pads
// with.  The first output of a push that starts at n0 frames has i0 >= n0, so it reaches back to frame n0 - (J - 1) at most:
// a stream carries its last J - 1 downmixed frames, as doubles (frames before the clip's start: zeros), and every output is
// the whole-clip fma chain over the same operands -- the same bits for any split.
#pragma once
#include "q3_enc_pcm_host.h"

namespace q3 {

// J - 1 at most: J = ceil((20 mr + 1) / up) with mr / up <= ENC_PCM_MAX_RATE / ENC_PCM_RATE for every rate enc_pcm_plan takes
constexpr int ENC_STREAM_PCM_CARRY = 20 * (ENC_PCM_MAX_RATE / ENC_PCM_RATE);

static inline long long enc_stream_pcm_ready(const EncPcmPlan& p, long long n) {
    const long long a = n * (long long)p.up - 1 - p.half;
    return a < 0 ? 0 : a / p.down + 1;
}

// samples a stream has handed to the op table after n input frames in all
static inline long long enc_stream_pcm_total(const EncPcmPlan& p, long long n, bool finished) {
    return finished ? enc_pcm_out_len(p, n) : enc_stream_pcm_ready(p, n);
}

// what one push of n_in frames hands on from a stream that had taken `before`
static inline long long enc_stream_pcm_new(const EncPcmPlan& p, long long before, long long n_in, bool finish) {
    return enc_stream_pcm_total(p, before + n_in, finish) - enc_stream_pcm_ready(p, before);
}

// Input frames of one entry of one push whose samples fit max_push at any phase, finishing or not.  With X = before * up:
// ceil((X + n up) / down) < (X + n up) / down + 1 and ready(before) >= (X - half) / down (0 >= that while ready is 0), so a
// push hands on fewer than (n up + half) / down + 1 samples, that is at most ceil((n up + half) / down); this is <= max_push
// when n up + half <= max_push down.  half <= 32 down at every rate from 8 kHz up (half = 10 max(up, down), up <= 3 down), so
// the result is at least floor((max_push - 32) down / up).
static inline int enc_stream_pcm_max_frames_in(long long max_push, const EncPcmPlan& p) {
    const long long room = max_push * (long long)p.down - p.half;
    if (room <= 0) return 0;
    const long long n = room / p.up;
    return n > 0x7fffffffLL ? 0x7fffffff : (int)n;
}

}  // namespace q3
