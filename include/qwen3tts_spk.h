/*
 * qwen3tts_spk.h -- C ABI of the MI355X speaker encoder (24 kHz mono audio -> one x-vector per clip).
 *
 * The second half of a cloned voice: an ECAPA-TDNN embedding of the reference clip's log-mel spectrogram, placed as one
 * row in the codec stream of the prefix (qwen3tts_text.h, tfe_build_prefix_spk).  Pinned by committed fixtures: the
 * log-mel front-end against float64 torch.stft plus the slaney filter bank, the network against transformers'
 * ECAPA_TimeDelayNet (models/qwen2_5_omni) in float64.  Recollection, not pinned (qwen_tts is not importable here): that
 * the checkpoint's speaker_encoder is that class at mel 128, channels 512/512/512/512/1536, Res2Net scale 8, SE 128,
 * attention 128 with enc_dim = the talker's hidden size; the mel parameters; the row's position in the prefix.  All three
 * are table / meta parameters of the weight container, not code.  No claim about voice similarity is made.
 *
 * Arithmetic: the log-mel in float64 on the device (reflect padding, periodic Hann window, direct DFT from host-made
 * double tables, sqrt(re^2 + im^2 + mag_eps), the filter bank as a tensor, log(max(mel, mel_floor))), rounded once to
 * float32; the network in fp32 on the exact-f32 MFMA convs.
 *
 * Caller-owned host buffers, synchronous, one caller thread per handle, no CPU fallback.
 */
#ifndef QWEN3TTS_SPK_H
#define QWEN3TTS_SPK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* weights: Q3TTSW1 container holding spk.* (weights.py: make_synthetic_spk / convert_speaker_encoder).
 * max_batch clips of at most max_samples samples per spk_embed call; the device buffers are sized for that at load.
 * NULL without a HIP device, on a malformed container, or when the buffers do not fit. */
void* spk_load(const char* weights, int max_batch, int max_samples);
void spk_free(void* h);
int spk_dim(void* h);           /* floats per embedding (the talker's hidden size) */
int spk_sample_rate(void* h);   /* 24000 */
int spk_min_samples(void* h);   /* the shortest clip spk_embed takes (1280) */
/* frames a clip of n_samples gives: 1 + (n + 2 * pad - n_fft) / hop; <0 when n <= pad or the result < 5 (the widest reflect
 * padding of the network, 4 columns, needs 5), or on a NULL handle */
int spk_frames(void* h, int n_samples);

/* B clips in one call.  pcm: the clips' samples concatenated (f32, nominally [-1, 1]); n_samples[B] their lengths.
 * out: f32 [B][spk_dim()].  Clip b gives the same bits alone and in any batch.
 * 0 ok; <0 with one logged line and the handle still usable: NULL handle or buffer, B outside 1..max_batch, a clip that
 * spk_frames refuses or that is longer than max_samples, a non-finite sample. */
int spk_embed(void* h, const float* pcm, const int32_t* n_samples, int B, float* out);

/* GPU milliseconds (HIP events on the handle's stream: upload to embedding) and kernel launches of the last spk_embed */
float spk_last_ms(void* h);
int spk_last_launches(void* h);

#ifdef __cplusplus
}
#endif

#endif /* QWEN3TTS_SPK_H */
