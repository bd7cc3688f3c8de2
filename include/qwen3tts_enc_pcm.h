/*
 * qwen3tts_enc_pcm.h -- the PCM front-end of the speech-tokenizer encoder (included by qwen3tts_enc.h; handles are
 * enc_load's).
 *
 * Interleaved PCM as a client has it -- s16le or f32le, 1..8 channels, an integer rate of 8000..192000 Hz
 * whose reduced factors up = 24000 / g, down = rate / g (g = gcd(rate, 24000)) are both <= 640: 8, 11.025, 12, 16, 22.05,
 * 24, 32, 44.1, 48, 88.2, 96 kHz among others -- is decoded (s16: v / 32768), downmixed (the mean of the channels) and
 * resampled to 24 kHz mono on the device, then encoded exactly as enc_encode encodes those samples.  The arithmetic is
 * pinned so that every host gets the same ids: scipy.signal.resample_poly's rules with its defaults (a Kaiser beta = 5
 * windowed sinc of 20 max(up, down) + 1 taps, zero padded at both ends, n_out = ceil(n up / down)), the taps designed on the
 * host in double, every output sample accumulated in float64 and rounded once to float32.  At 24 kHz there is
 * no filter: the downmixed sample rounded to float32. */
#ifndef QWEN3TTS_ENC_PCM_H
#define QWEN3TTS_ENC_PCM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ENC_PCM_S16 0
#define ENC_PCM_F32 1
/* frames a clip of n_in input frames at `rate` gives after the front-end (<0: refused) */
int enc_pcm_frames(void* h, int n_in, int rate);
/* B clips, one format / channel count / rate per call; pcm: the clips' interleaved frames concatenated (n_in[b] frames of
 * `channels` samples each).  Outputs and errors as enc_encode: 0, or <0 with one logged line and the handle still usable --
 * also for a format, channel count or rate outside the above, a clip whose 24 kHz length is 0 or above max_samples, a
 * non-finite f32 sample.  Clip b gives the same bits alone and in any batch. */
int enc_encode_pcm(void* h, const void* pcm, int format, int channels, int rate, const int32_t* n_in, int B,
                   int64_t* codes_out, int max_frames, int32_t* n_frames);

#ifdef __cplusplus
}
#endif

#endif /* QWEN3TTS_ENC_PCM_H */
