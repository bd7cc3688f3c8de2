/*
 * qwen3tts_enc_stream.h -- carry-state streaming encode (enc_stream_*), the encoder's counterpart of voc_incr_*
 * (qwen3tts_voc.h).  Included by qwen3tts_enc.h; the entry points live in a file of their own so that the list of
 * whole-clip entry points in qwen3tts_enc.h stays what it was.
 *
 * Every op of `enc.program` is causal (causal convs, causal sliding-window attention, per-column norm, per-frame RVQ), so
 * frame f depends on samples < (f + 1) * hop only (hop = enc_samples_per_frame).  A stream keeps, per op with a receptive
 * field, the columns its next output still reads ("Streaming encode") -- constant memory whatever the clip's
 * length -- and a push runs the op table over the new columns only.
 *
 * Hand-out rule (an identity of the table): after pushes totalling n samples a stream has handed out exactly
 * floor(n / hop) frames; the push that finishes the stream pads the leftover samples as enc_encode pads a clip's end
 * (zeros, or the last column where the op replicates) and brings the total to enc_frames(n).  A stream finished with
 * 0 samples gives 0 frames; a push may give 0 frames.
 *
 * Joined, a stream's ids are the same bits for any split of its samples across pushes, any other streams in the same
 * calls and any stream index.  Against enc_encode of the same clip: the same frame count, embeddings within rounding
 * (the attention rotates q and k by their offset inside the window instead of the absolute column once the stream is
 * longer than the window: not the same bits), ids equal except at near-ties.  Exact-fp32 arithmetic only.
 *
 * One caller thread per encoder handle and the objects on it; every entry point binds the thread to the handle's device.
 * All device memory is allocated by enc_stream_create (the carry rows of the PCM front-end, qwen3tts_enc_stream_pcm.h, by
 * its first push; a clip is fed by enc_stream_push or by enc_stream_push_pcm, not both: the other one is refused until
 * enc_stream_reset).
 */
#ifndef QWEN3TTS_ENC_STREAM_H
#define QWEN3TTS_ENC_STREAM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* max_streams independent streams on the encoder handle `enc`; a push gives a stream at most max_push_samples samples.
 * Entries of a push with the same column counts at every level run together, up to the handle's max_batch at a time.
 * NULL: no memory, a NULL handle, counts <= 0, or a table holding an op that cannot be carried (logged). */
void* enc_stream_create(void* enc, int max_streams, int max_push_samples);
void enc_stream_free(void* s); /* before its encoder handle */
/* stream `stream` starts a new clip (its state is the causal padding again).  0 / <0 bad index */
int enc_stream_reset(void* s, int stream);

/* frames the push described by (streams, n_new, finish) hands out in all; <0 when enc_stream_push would refuse it for a
 * reason other than the samples' values or the capacity */
int enc_stream_push_max_frames(void* s, int n, const int32_t* streams, const int32_t* n_new, const int32_t* finish);

/* n entries: stream streams[i] takes n_new[i] samples (0..max_push_samples) and, where finish[i] != 0, ends (finish may be
 * NULL: none ends).  pcm: the entries' new samples concatenated.  codes_out receives the packed [frames][nq] int64 rows,
 * entry after entry, in the layout enc_encode writes; entry i's rows are offsets[i] .. offsets[i + 1] (offsets [n + 1]).
 * 0 ok; <0 with one logged line: a bad stream index or one named twice, n_new outside its range, a non-finite sample, a
 * push to a finished stream without a reset, out_capacity_frames below enc_stream_push_max_frames.  On any of these
 * nothing is written and no stream changes: the same push can be retried. */
int enc_stream_push(void* s, int n, const int32_t* streams, const float* pcm, const int32_t* n_new, const int32_t* finish,
                    int64_t* codes_out, int64_t out_capacity_frames, int64_t* offsets);

float enc_stream_last_ms(void* s);        /* GPU milliseconds of the last push (HIP events: upload to codes) */
int enc_stream_last_launches(void* s);    /* kernel launches of the last push */
int64_t enc_stream_state_bytes(void* s);  /* carried state of one stream */
int64_t enc_stream_device_bytes(void* s); /* everything the object holds; fixed by create */

#ifdef __cplusplus
}
#endif
#endif /* QWEN3TTS_ENC_STREAM_H */
