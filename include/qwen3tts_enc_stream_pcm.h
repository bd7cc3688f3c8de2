/*
 * qwen3tts_enc_stream_pcm.h -- the PCM front-end of the streaming encode: enc_stream_push for audio as a client has it.
 * Included by qwen3tts_enc.h; the objects are enc_stream_create's (qwen3tts_enc_stream.h), the formats, channel counts and
 * rates those of enc_encode_pcm (qwen3tts_enc_pcm.h).
 *
 * A push brings interleaved s16le / f32le frames of 1..8 channels at the client's rate; they are decoded, downmixed and
 * resampled to 24 kHz on the device and go straight into the streaming encode, without returning to the host.
 *
 * Bit-equality contract.  A stream keeps the last per_phase - 1 downmixed input frames as doubles (at most 160; none at
 * 24 kHz), so every 24 kHz sample is enc_encode_pcm's float64 fma chain over the same operands, rounded once: joined, the
 * samples a stream hands to the encoder are the same bits as the samples enc_encode_pcm prepares for the whole clip, for
 * any split of the clip's frames across pushes (empty pushes, single frames, a finish with no new frame), any other
 * streams in the same calls and any stream index.  The ids are therefore the bits of enc_stream_push fed those samples,
 * and enc_stream_push's own contracts carry over.
 *
 * Hand-out rule.  With g = gcd(rate, 24000), up = 24000 / g, down = rate / g, half = 10 max(up, down) (0 at 24 kHz): after
 * n input frames an unfinished stream has handed the encoder
 *     ready(n) = n up - 1 - half < 0 ? 0 : (n up - 1 - half) / down + 1
 * samples, the outputs whose newest input frame has arrived; the finishing push brings that to ceil(n up / down), the
 * missing frames read as zeros, as enc_encode_pcm pads a clip's end.  Frames follow from the samples by enc_stream_push's
 * rule: floor(samples / hop) while the stream runs, enc_frames(samples) after the finish; 0 frames in all give 0 samples
 * and 0 frames.
 *
 * Memory rule.  enc_stream_create allocates nothing for the front-end, and enc_stream_state_bytes / enc_stream_device_bytes
 * do not count it.  The first enc_stream_push_pcm of an object allocates two carry rows of 160 doubles per stream and the
 * launch metadata (enc_stream_pcm_device_bytes: 0 before, constant after, whatever the clips' lengths and rates); the tap
 * tables and the payload buffer are the encoder handle's, shared with enc_encode_pcm under its rules (four tables kept, the
 * payload buffer as large as the largest payload seen).
 */
#ifndef QWEN3TTS_ENC_STREAM_PCM_H
#define QWEN3TTS_ENC_STREAM_PCM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 24 kHz samples a stream has handed to the encoder after n_in_total input frames at `rate` (finished != 0: after its
 * finishing push): the rule above.  <0: a rate enc_encode_pcm refuses, or a negative count */
int64_t enc_stream_pcm_samples(void* s, int rate, int64_t n_in_total, int finished);
/* the most input frames one entry of one push may bring at `rate`, so that its samples fit max_push_samples at any phase
 * of the stream, finishing or not; at least (max_push_samples - 32) * down / up.  <0: refused rate */
int enc_stream_pcm_max_frames_in(void* s, int rate);
/* frames the push described hands out in all; <0 when enc_stream_push_pcm would refuse it for a reason other than the
 * samples' values or the capacity */
int enc_stream_push_pcm_max_frames(void* s, int n, const int32_t* streams, int format, int channels, int rate,
                                   const int32_t* n_in, const int32_t* finish);
/* enc_stream_push from PCM: n entries, one format / channel count / rate per call; stream streams[i] takes n_in[i] input
 * frames (0 .. enc_stream_pcm_max_frames_in) and, where finish[i] != 0, ends.  pcm: the entries' interleaved frames
 * concatenated.  codes_out, out_capacity_frames and offsets as enc_stream_push.  A stream remembers the format, channels and
 * rate of its first push since enc_stream_reset.  0 ok; <0 with one logged line, nothing written and no stream changed (the
 * same push can be retried): another format, channel count or rate than the clip began with; a clip enc_stream_push has fed
 * (and enc_stream_push refuses a clip this call has fed); n_in outside its range; a non-finite f32 sample; a finished
 * stream; whatever enc_encode_pcm refuses of a format, channel count or rate; every refusal of enc_stream_push. */
int enc_stream_push_pcm(void* s, int n, const int32_t* streams, const void* pcm, int format, int channels, int rate,
                        const int32_t* n_in, const int32_t* finish, int64_t* codes_out, int64_t out_capacity_frames,
                        int64_t* offsets);
/* device memory of the front-end: carry rows and launch metadata; 0 until the first enc_stream_push_pcm */
int64_t enc_stream_pcm_device_bytes(void* s);

#ifdef __cplusplus
}
#endif
#endif /* QWEN3TTS_ENC_STREAM_PCM_H */
