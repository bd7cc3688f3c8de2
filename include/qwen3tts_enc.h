/*
 * qwen3tts_enc.h -- C ABI of the MI355X speech-tokenizer encoder (24 kHz mono audio -> 16-group codec ids, fp32).
 *
 * The encode half of the 12 Hz speech tokenizer: what the reference's scripts/encode_reference_audio.py computes on a
 * CPU through qwen_tts to write a voice-clone prompt's ref_codec_tokens.npy ([T][16] int64).  The layer list is not in
 * the reference; the library executes the op table stored in the weight container (`enc.program`, DESIGN.md "Speech
 * tokenizer encoder"), whose semantics are pinned to transformers' MimiModel.encode(..., num_quantizers=16): SEANet
 * encoder (causal convs, ELU, strided downsampling), sliding-window transformer, replicate-padded 25 -> 12.5 Hz
 * downsample, split residual VQ (1 semantic + 15 acoustic codebooks).  That Qwen3-TTS's tokenizer encoder IS that
 * module is recollection (qwen_tts is not importable here); parity with a real checkpoint is unpinned.
 *
 * Codes come out in the layout voc_synthesize reads: [frames][16] int64, the semantic id first.  A clip of n samples
 * gives enc_frames(n) = ceil(n / enc_samples_per_frame()) frames (MimiModel.get_encoded_length).
 *
 * Caller-owned host buffers, synchronous, one caller thread per handle, no CPU fallback.
 */
#ifndef QWEN3TTS_ENC_H
#define QWEN3TTS_ENC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* weights: Q3TTSW1 container holding enc.* (weights.py: make_synthetic_enc / convert_speech_tokenizer_encoder).
 * max_batch clips of at most max_samples samples per enc_encode call; the device buffers are sized for that at load.
 * NULL without a HIP device, on a malformed table, or when the buffers do not fit. */
void* enc_load(const char* weights, int max_batch, int max_samples);
void enc_free(void* h);
int enc_num_quantizers(void* h);     /* ids per frame (16) */
int enc_sample_rate(void* h);        /* 24000 */
int enc_samples_per_frame(void* h);  /* hop: the product of the strides (1920) */
int enc_frames(void* h, int n_samples);   /* frames a clip of n_samples gives (<0: n_samples <= 0 or NULL handle) */

/* B clips in one call.  pcm: the clips' samples concatenated (f32, nominally [-1, 1]); n_samples[B] their lengths.
 * codes_out: int64 [B][max_frames][nq]; clip b's enc_frames(n_samples[b]) rows are its ids, the rows after them are -1;
 * n_frames[B] receives the frame counts.  Clip b gives the same bits alone and in any batch.
 * 0 ok; <0 with one logged line: NULL handle or buffer, B outside 1..max_batch, a length <= 0 or > max_samples, a
 * non-finite sample, max_frames below a clip's frame count. */
int enc_encode(void* h, const float* pcm, const int32_t* n_samples, int B, int64_t* codes_out, int max_frames,
               int32_t* n_frames);

/* GPU milliseconds of the last enc_encode / enc_encode_pcm (HIP events on the handle's stream: upload -- the front-end
 * included -- to codes) */
float enc_last_ms(void* h);

#ifdef __cplusplus
}
#endif

/* Streaming encode: clips of any length in constant memory, ids as the samples arrive */
#include "qwen3tts_enc_stream.h"
/* PCM front-end: s16 / f32 PCM of any channel count at the client's rate, decoded, downmixed and resampled on the device */
#include "qwen3tts_enc_pcm.h"
/* The two together: a stream's pushes as s16 / f32 PCM at the client's rate, the same samples bit for bit */
#include "qwen3tts_enc_stream_pcm.h"
/* The PCM front-end alone: the 24 kHz samples enc_encode_pcm encodes, for the speaker encoder (qwen3tts_spk.h) */
#include "qwen3tts_enc_resample.h"

#endif /* QWEN3TTS_ENC_H */
