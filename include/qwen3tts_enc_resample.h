/*
 * qwen3tts_enc_resample.h -- the encoder's PCM front-end on its own (included by qwen3tts_enc.h; handles are enc_load's).
 *
 * The 24 kHz mono samples that enc_encode_pcm encodes (qwen3tts_enc_pcm.h: decoded, downmixed, resampled in float64 on the
 * device and rounded once to float32), handed back bit for bit.  One resampler for both halves of a cloned voice: the codec
 * prompt (enc_encode_pcm) and the speaker embedding (qwen3tts_spk.h, spk_embed of these samples).
 */
#ifndef QWEN3TTS_ENC_RESAMPLE_H
#define QWEN3TTS_ENC_RESAMPLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* pcm, format, channels, rate, n_in, B as enc_encode_pcm takes them.  out: f32 [B][out_pitch], clip b's n_out[b] samples
 * from out + b * out_pitch (the floats after them are left as they were).  0, or <0 with one logged line and the handle
 * still usable: every refusal of enc_encode_pcm, and a clip that gives more than out_pitch samples. */
int enc_resample_pcm(void* h, const void* pcm, int format, int channels, int rate, const int32_t* n_in, int B, float* out,
                     int out_pitch, int32_t* n_out);

#ifdef __cplusplus
}
#endif

#endif /* QWEN3TTS_ENC_RESAMPLE_H */
