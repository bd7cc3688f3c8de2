/*
 * qwen3tts_voc.h -- C ABI of the MI355X vocoder library (codec ids -> 24 kHz waveform, fp32).
 *
 * The reference has no C ABI here: dual_npu/vocoder_server.py:67-71 calls onnxruntime
 * (`sess.run(None, {'audio_codes': i64[1,64,16]})[0].flatten()`), the graph being the traced
 * Qwen3TTSTokenizerV2 decoder of scripts/export_vocoder_traced.py:38-52 (input [B,T,16] int64,
 * permuted to [B,16,T]; output wav.squeeze(1), length T * total_upsample = T * 1920).  voc_decode
 * is that call; voc_synthesize is VocoderServer.synthesize + the int16 rule
 * (vocoder_server.py:73-121,175) including its chunk-length quirk.
 *
 * The decoder's layer list is NOT in the reference: the library executes
 * the op table stored in the weight container (`voc.program`, DESIGN.md "Vocoder program"), so a
 * real checkpoint only needs converting, not a rebuild.  The table's semantics are pinned to the
 * importable implementation of the decoder family (transformers' Qwen3OmniMoeCode2Wav + Mimi's split
 * RVQ: tests/golden/make_code2wav_golden.py).  That family's transposed convs trim kernel - stride
 * samples at BOTH ends, so a decode of T frames returns fewer than T * 1920 samples (64 frames ->
 * 122 325): like the ONNX model's output tensor, voc_decode's rows are voc_chunk_samples() long, and
 * the slices the reference takes of them (`audio[:n * 1920]`, vocoder_server.py:81,98-99) follow
 * numpy's rule -- as long as what is there.
 *
 * Caller-owned host buffers, synchronous, one caller thread per handle, no CPU fallback.
 */
#ifndef QWEN3TTS_VOC_H
#define QWEN3TTS_VOC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define Q3VOC_SAMPLES_PER_TOKEN 1920 /* vocoder_server.py:30 */
#define Q3VOC_SAMPLE_RATE 24000      /* vocoder_server.py:29 */

/* weights: Q3TTSW1 container holding voc.*.  chunk_tokens: frames per decode call (the ONNX model's
 * fixed input length, 64 in the reference: vocoder_server.py:45-46); max_batch chunks per call. */
void* voc_load(const char* weights, int chunk_tokens, int max_batch);
void voc_free(void* v);
int voc_chunk_tokens(void* v);
int voc_samples_per_token(void* v);   /* decoder.total_upsample (export_vocoder_traced.py:46): the product of the strides */
int voc_chunk_samples(void* v);      /* samples one decode of chunk_tokens frames returns (<= chunk_tokens * samples_per_token) */

/* codes[B][chunk_tokens][16] int64 (ids 0..2047; out-of-range ids embed as zeros) ->
 * out[B][voc_chunk_samples()] f32 in [-1, 1] (the ONNX output tensor's shape).  0 ok / <0 error. */
int voc_decode(void* v, const int64_t* codes, int B, float* out);

/* VocoderServer.synthesize + int16 conversion for one utterance: codes[n][16] -> out samples.
 * out must hold voc_synthesize_max_samples(n) int16.  Returns 0 and *n_samples, or <0.
 * It is voc_synthesize_batch with one utterance: the same chunk walk, decodes, placement and int16 rule on the device, so the
 * two return the same bits for the same utterance.  On the split arithmetic a call in which an activation leaves the fp16
 * range is redone whole on the exact path (voc_synthesize_batch's rule).  Sets voc_last_batch_ms / voc_last_batch_chunks,
 * not voc_last_decode_ms.
 * (n > chunk_tokens walks chunks with a 16-frame overlap: needs chunk_tokens > 32.)
 * In the exact-fp32 mode (voc_set_exact_fp32(1)) a chunk of fewer than chunk_tokens frames (an utterance's tail, or a short
 * utterance) is decoded at its own length + 1 pad frame, rounded up to 8, instead of the reference's zero-padded chunk_tokens:
 * the decoder is causal but for a quarter frame of look-ahead, and every op picks its kernel from the full chunk's length, so
 * the samples the walk keeps are bit-identical.  The split mode (the default) always pads to chunk_tokens, since its
 * fp16-range redo is per call (env Q3_VOC_FULL_CHUNKS=1: pad as the reference in both modes). */
int voc_synthesize(void* v, const int64_t* codes, int n_tokens, int16_t* out, int32_t* n_samples);
/* same, float output before the int16 rule */
int voc_synthesize_f32(void* v, const int64_t* codes, int n_tokens, float* out, int32_t* n_samples);
int voc_synthesize_max_samples(void* v, int n_tokens);

/* The same for U utterances in one call (BASELINE configs[2]: "streaming overlap-crossfade vocoder" at batch): codes =
 * the utterances' frames concatenated ([sum n_tokens][16]); the chunks of ALL utterances are decoded max_batch at a time
 * and every utterance's chunk walk -- 64-frame chunks stepping by 48, the 16-frame linear cross-fade, the appended short
 * tail chunk (vocoder_server.py:84-117) -- is assembled on the device, bit-identical to voc_synthesize[_f32] per
 * utterance.  out holds voc_synthesize_batch_max_samples() samples (out_capacity of them are the caller's);
 * utterance u's samples are out[offsets[u] .. offsets[u+1]) (offsets has U + 1 entries).  0 ok / <0 error. */
int voc_synthesize_batch(void* v, const int64_t* codes, const int32_t* n_tokens, int U, int16_t* out, int64_t out_capacity,
                         int64_t* offsets);
int voc_synthesize_batch_f32(void* v, const int64_t* codes, const int32_t* n_tokens, int U, float* out, int64_t out_capacity,
                             int64_t* offsets);
int64_t voc_synthesize_batch_max_samples(void* v, const int32_t* n_tokens, int U);
/* GPU milliseconds and decoded chunks of the last voc_synthesize* or voc_synthesize_batch* call */
float voc_last_batch_ms(void* v);
int voc_last_batch_chunks(void* v);

/* Streaming chunk walk: the walk of voc_synthesize_batch fed frame by frame, for many utterances ("streams", e.g. one per slot of
 * the frame loop) at once.  voc_stream_create(voc, max_streams) -> NULL on failure; free the stream object before its vocoder
 * handle.  Every stream starts empty; voc_stream_reset starts a new utterance in it (dropping an unfinished one).
 *
 * voc_stream_push: n entries; entry i gives stream streams[i] (each stream at most once per call) n_new[i] >= 0 more frames --
 * codes holds the entries' new frames concatenated, [sum n_new][16] -- and finish[i] != 0 ends its utterance (finish may be NULL:
 * none ends).  Entry i's samples land in out[offsets[i] .. offsets[i+1]) (offsets has n + 1 entries); out_capacity samples of out
 * are the caller's, voc_stream_push_max_samples() returns how many the same push hands out (<0: the push is invalid).
 *  - Bits: per stream, the samples of all pushes from a reset to its finish push, joined, are voc_synthesize_f32 (push_f32) /
 *    voc_synthesize (push) of all its frames, bit for bit, however the frames were split across pushes and whatever other
 *    streams shared the calls.  On the split arithmetic (voc_set_exact_fp32(0)) a push in which an activation leaves the fp16
 *    range is redone exact, like one voc_synthesize_batch call -- the samples of earlier pushes stay as they were handed out, so
 *    the joined result can then differ from a whole-utterance call; on the exact path it never does.
 *  - Latency: after a push that does not finish a stream, that stream has handed out every sample no later chunk can change:
 *    the walk assembled so far minus its last 16 * samples_per_token samples (the next chunk's cross-fade), nothing before 64
 *    frames.  A full chunk_tokens chunk is decoded in the push that completes it; the tail chunk(s) -- the reference's
 *    redundant short chunk, the plain append of a chunk shorter than the overlap -- in the finish push, which hands out all the
 *    rest.  A stream that finishes with 0 frames gives 0 samples.
 *  - Batching: the chunks that become decodable in one push are decoded together across its streams, max_batch per call and
 *    one decode length per call (voc_synthesize_batch's grouping); a push that completes no chunk decodes nothing.  The
 *    unfinished tail of every stream stays on the device; placement, cross-fade, the int16 rule and the packing run there.
 *  - Errors (<0): a bad stream index or one named twice, n_new < 0, a push to a finished stream without a reset, out_capacity
 *    below what the push hands out.  Nothing is written to out and no stream changes: the same push can be retried.
 *  - Threads: one caller thread at a time per vocoder handle and its stream objects; entry points bind the thread to the
 *    handle's device. */
void* voc_stream_create(void* voc, int max_streams);
void voc_stream_free(void* s);
int voc_stream_reset(void* s, int stream);
int64_t voc_stream_push_max_samples(void* s, int n, const int32_t* streams, const int32_t* n_new, const int32_t* finish);
int voc_stream_push(void* s, int n, const int32_t* streams, const int64_t* codes, const int32_t* n_new, const int32_t* finish,
                    int16_t* out, int64_t out_capacity, int64_t* offsets);
int voc_stream_push_f32(void* s, int n, const int32_t* streams, const int64_t* codes, const int32_t* n_new, const int32_t* finish,
                        float* out, int64_t out_capacity, int64_t* offsets);
/* the last push: decode calls, chunks decoded, GPU milliseconds of its decodes and placement */
int voc_stream_last_decodes(void* s);
int voc_stream_last_chunks(void* s);
float voc_stream_last_ms(void* s);

/* Carry-state incremental decode: the third way to drive the vocoder, next to voc_decode and the chunk walk.  The decoder is run
 * as a stateful stream -- every op with a receptive field keeps, per stream, the last columns of its input on the device (convs
 * (k - 1) * dilation columns, transposed convs k / s - 1, attention the last window - 1 columns of k | v and the stream's absolute
 * position for RoPE) -- so a push decodes only its new frames and hands their samples out at once.  Joined, a stream's samples
 * are ONE seamless whole-utterance decode of all its frames, of any length: no chunks, no overlap decoded twice, no cross-fade.
 * This is NOT what voc_synthesize* returns for more than chunk_tokens frames (the reference's walk cross-fades chunks that each
 * start from silence); up to chunk_tokens frames the two agree to rounding.
 * voc_incr_create(voc, max_streams) -> NULL on failure (also: a table whose transposed convs do not trim k - s samples on the
 * right cannot be streamed; the 'both' and 'right' trims can).  Free it before its vocoder handle.  Entries, codes, finish, out,
 * out_capacity and offsets are voc_stream_push's.
 *  - Samples per push: let S(n) = voc_incr_samples(voc, n) be the length of a whole decode of n frames -- the table's convt_out
 *    chain applied to n (each transposed conv turns L columns into (L - 1) * s + k - lt - rt), 0 where that is not positive; at
 *    the default table with both trims S(8) = 14 805 and S(64) = 122 325.  After pushes totalling n frames a stream has handed
 *    out exactly S(n) samples: an identity of the table, not a measurement.  The finish push adds none (the model defines nothing
 *    past S(N)); a stream that finishes with 0 frames gives 0 samples.
 *  - Invariance: joined per stream, the samples are the same bits for any split of the frames across pushes, any n_new pattern,
 *    any set of other streams in the same calls, and any stream index: every launcher rule that looks at a length reads the
 *    full-chunk length, and a column's sums depend on neither its tile nor its batch.
 *  - Arithmetic: the exact-fp32 kernels by default, whatever voc_set_exact_fp32 has set for the process; voc_set_fused_units applies,
 *    with the value it had when the push began (the settings' contract, at voc_set_exact_fp32).
 *    voc_incr_set_arithmetic (below) moves one object to the split-fp16 convolutions.
 *  - Limits: 0 <= n_new <= chunk_tokens per entry and push; frames per stream unbounded (2^31, the RoPE position).  Device memory
 *    is constant: per stream the carried columns, voc_incr_state_bytes() = 5 193 984 B (4.95 MiB) at the default table (of which
 *    4.44 MiB are the eight attention windows); per handle work buffers for one push of chunk_tokens frames x max_batch entries
 *    and the packed output of max_streams entries, all allocated by voc_incr_create (voc_incr_device_bytes(): the total).
 *  - Batching: entries of one push with the same n_new are decoded together, up to max_batch per launch sequence; distinct
 *    n_new values run one after another, and so do a stream's first frames (its first transposed-conv outputs fall before
 *    sample 0, so it takes fewer columns than a running stream).  Packing and the int16 rule run on the device.
 *  - Errors (<0): a bad stream index or one named twice, n_new outside 0..chunk_tokens, a push to a finished stream without a
 *    reset, out_capacity below what the push hands out.  Nothing is written to out and no stream changes: the same push can be
 *    retried.
 *  - Threads: one caller thread at a time per vocoder handle and the objects on it; entry points bind the thread to the handle's
 *    device. */
void* voc_incr_create(void* voc, int max_streams);
void voc_incr_free(void* s);
int voc_incr_reset(void* s, int stream);
int64_t voc_incr_push_max_samples(void* s, int n, const int32_t* streams, const int32_t* n_new, const int32_t* finish);
int voc_incr_push(void* s, int n, const int32_t* streams, const int64_t* codes, const int32_t* n_new, const int32_t* finish,
                  int16_t* out, int64_t out_capacity, int64_t* offsets);
int voc_incr_push_f32(void* s, int n, const int32_t* streams, const int64_t* codes, const int32_t* n_new, const int32_t* finish,
                      float* out, int64_t out_capacity, int64_t* offsets);
/* the last push: GPU milliseconds and kernel launches */
float voc_incr_last_ms(void* s);
int voc_incr_last_launches(void* s);
int64_t voc_incr_samples(void* voc, int64_t n_frames);   /* S(n); <0: bad arguments */
int64_t voc_incr_state_bytes(void* s);    /* device bytes one stream's carried state takes */
int64_t voc_incr_device_bytes(void* s);   /* device bytes the object holds: fixed by voc_incr_create (+ the first switch to split) */

/* Arithmetic of ONE incremental object, independent of voc_set_exact_fp32: 0 (default) the exact-fp32 kernels, 1 the split-fp16
 * convolutions (voc_set_exact_fp32's note) wherever a conv is built for them; embedding, depthwise conv, norm, GLU and attention
 * are f32 in both, a conv with a weight beyond the fp16 range stays exact, and a residual unit runs as its two convs.
 * voc_incr_set_arithmetic is accepted only while every stream of the object is idle (fresh, reset, or finished): otherwise it
 * returns <0 and changes nothing.  -> the mode in effect.  The first switch to 1 allocates the second history buffer, the fp16
 * planes and the per-entry flags (voc_incr_device_bytes grows once; an object that never switches holds what it always held).
 * The carried history stays f32 -- voc_incr_state_bytes keeps its value -- and the planes are rebuilt from it every push.
 *  - Invariance: as long as no entry is redone, a stream's joined samples are the same bits for any split of the frames, any
 *    n_new pattern, any neighbours and any stream index, as in exact mode (a column's sums depend on neither tile nor batch).
 *  - Overflow: a push is a transaction per entry.  The history is double-buffered per stream; every kernel that writes planes
 *    flags the entry whose value leaves +-65504 (or is a NaN).  An unflagged entry commits.  A flagged entry's push is dropped
 *    and decoded again, from the same uncommitted history, on the exact-fp32 kernels (logged once per object), and then commits:
 *    the split arithmetic never degrades a result silently.  An entry's bits never depend on whether a neighbour overflowed.
 *    After a redo the stream's joined result depends on which push was redone (split and exact columns differ in rounding):
 *    voc_stream_push's rule for the split path.  The flags also cover columns a push computes and drops (the outputs of history
 *    columns in front of a one-tap conv's new ones): a redo can come from those alone; it costs time, never accuracy.
 * voc_incr_last_split_launches: conv launches of the last push that ran on the fp16 MFMA path (0 in exact mode);
 * voc_incr_last_redone: entries of the last push that were redone on the exact path. */
int voc_incr_set_arithmetic(void* s, int split);
int voc_incr_arithmetic(void* s);
int voc_incr_last_split_launches(void* s);
int voc_incr_last_redone(void* s);

/* Snapshots of a stream's carried state.  A stream's samples depend on its frames and on nothing else, so the state it carries
 * after frames P is a function of P and the arithmetic alone: it can be computed once, saved, and copied into any stream that is
 * to continue P (a voice's codec prompt in front of many utterances).  The pool belongs to the vocoder HANDLE: every incremental
 * object on a handle lays a stream's state out the same way, so a slot saved by one object serves the others.
 *  - voc_incr_snapshots(voc, n_slots): n_slots > 0 reserves a device pool of n_slots x voc_incr_state_bytes() (5 193 984 B per slot
 *    at the default table), 0 releases it; either way every snapshot is dropped.  -> n_slots; <0 with nothing changed on a
 *    negative n_slots or no memory.  Legal at any time between calls.  voc_free frees the pool, voc_incr_free does not touch it.
 *  - voc_incr_save(s, stream, slot): the stream's committed history (under double buffering the buffer its parity selects) goes
 *    into the slot, with the frames the stream has taken and the arithmetic of s, replacing what the slot held.  Any unfinished
 *    stream can be saved, a fresh one too (0 frames: restoring it is voc_incr_reset).  <0 with nothing changed: a bad stream or
 *    slot, a finished stream, no pool.  Runs on the handle's stream: no further stream, event or hardware queue.
 *  - voc_incr_restore(s, n, streams, slots): stream streams[i] becomes a running, unfinished stream whose history and frame count
 *    are those of slots[i]; the utterance it held is dropped, as by a reset.  A slot may be named several times (one voice into many
 *    streams), a stream at most once.  All n entries are copied by ONE kernel launch; a double-buffered object gets both of its
 *    history buffers written, since an op that a push does not reach reads the other buffer next time (voc_incr_reset clears both
 *    for the same reason).  Every entry is checked before anything changes -- <0 with every stream as it was: a bad index, a
 *    stream named twice, an empty slot, a slot saved under the other arithmetic, no pool.
 *  - voc_incr_snapshot_frames(voc, slot): the frames the slot holds; -1: an empty slot or a bad argument.
 *  - voc_incr_last_restore_ms(s): GPU milliseconds of the last voc_incr_restore (HIP events on the handle's stream).
 *  - Contract: let stream a take frames P (T of them, in any pushes); save it; restore the slot into stream b of any object on the
 *    same handle that runs the same arithmetic; push frames U into b in any split, beside any neighbours.  b's samples, joined, are
 *    bit for bit samples [S(T), S(T + |U|)) of ONE uninterrupted stream fed [P ; U] -- always in exact mode, in split mode as long
 *    as no push on either side is redone on the exact path (voc_incr_set_arithmetic's rule).  After pushes totalling m frames b has
 *    handed out exactly S(T + m) - S(T) samples.  Nothing else about b is special: its launches are grouped by its frame count (with
 *    T >= 1 it is a running stream, not a first push), the 2^31 frame limit counts T, voc_incr_set_arithmetic sees it as running.
 *  - Snapshots survive voc_incr_set_arithmetic and voc_incr_free and stay tagged with the arithmetic they were saved under.
 *    voc_set_fused_units changes the last bit of exact-mode results: a snapshot taken under one setting and continued under the
 *    other is the caller's affair (the library does not tag it). */
int voc_incr_snapshots(void* voc, int n_slots);
int voc_incr_save(void* s, int stream, int slot);
int voc_incr_restore(void* s, int n, const int32_t* streams, const int32_t* slots);
int64_t voc_incr_snapshot_frames(void* voc, int slot);
float voc_incr_last_restore_ms(void* s);

/* Arithmetic of the convolutions.  Default (0): split precision -- every f32 operand (weights once at load,
 * activations in the producing kernel's epilogue) is carried as two fp16 terms (22 mantissa bits) and each
 * product costs three fp16 MFMAs with f32 accumulation.  1: the exact-f32 MFMA (v_mfma_f32_32x32x2_f32)
 * everywhere.  Measured on MI355X against a float64 evaluation of the same table: max error 2.2e-7 (split)
 * vs 4.0e-7 (exact f32 MFMA) vs 2.1e-7 (torch CPU f32) of full scale -- the split path is fp32-grade, and
 * 2.8x faster at 32 chunks.  Values beyond the fp16 range cannot be split: an op with such a weight stays
 * exact, and a call in which an activation leaves the range is redone on the exact path before it returns (voc_decode,
 * voc_synthesize*: the whole call).  Env Q3_VOC_EXACT=1 selects the exact path at load.
 * The settings' contract (this call, voc_set_fused_units, voc_set_max_workgroups): the setting is process-wide -- one value for
 * every handle -- and may be set from any thread, also while other threads are inside the library.  It takes effect from the next
 * voc_* call on: every call reads the settings once, as it begins, and a call in flight finishes under the settings it started
 * with -- planning, every launch and the fp16-range check of one call see one arithmetic, so the redo above cannot be missed. */
int voc_set_exact_fp32(int on);

/* 1 (default): on the exact-f32 path a residual unit of the 96- / 192-channel decoder blocks (Snake, dilated 7-tap
 * conv, Snake, 1x1 conv, + input) runs as ONE launch whose intermediate stays in MFMA accumulators; 0: one launch
 * per conv (the 1x1 conv then sums its channels in a different order: results differ in the last f32 bit).
 * Process-wide, any thread, from the next voc_* call on (voc_set_exact_fp32's contract). */
int voc_set_fused_units(int on);

/* Cap the workgroups each vocoder kernel launch occupies (0 = one per output tile, the default and the fastest for a decode that
 * has the GPU to itself; -1 = one per compute unit of the current device).  With a cap the kernels walk their tiles persistently
 * -- same tiles, same sums, same bits -- and leave registers and LDS of every compute unit to a concurrently running frame loop
 * (talker / code predictor), which is latency-bound and otherwise finds room only in the tails of the vocoder's launches.  Measured
 * on MI355X, 32 utterances, frame loop of step s + 1 beside the decode of step s: exactly one workgroup per CU is the optimum
 * (the decode alone 89 -> 125 ms, the frame step beside it 2.40 -> 2.9 ms instead of starving, the whole step 244 -> 209 ms with the
 * frame loop's waves at raised priority, which the library's kernels set themselves); 320 / 384 / 512 / 768 workgroups: 239 / 228 /
 * 234 / 245 ms.  Returns the cap in effect.
 * Process-wide, any thread, from the next call on (voc_set_exact_fp32's contract) -- the next voc_*, and the next enc_* / spk_*
 * call too: the encoders' convs run on the vocoder's exact-f32 launcher and follow the cap.  A call in flight keeps its grid.
 * (n = -1 asks the HIP runtime for the current device's compute units, on the calling thread.) */
int voc_set_max_workgroups(int n);

/* GPU milliseconds of the last voc_decode (HIP events on the library's stream; voc_synthesize* leave it alone) and its FLOP
 * count. */
float voc_last_decode_ms(void* v);
double voc_decode_flops(void* v, int B);

#ifdef __cplusplus
}
#endif
#endif /* QWEN3TTS_VOC_H */
