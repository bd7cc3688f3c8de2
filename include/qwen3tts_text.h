/*
 * qwen3tts_text.h -- C ABI of the text front-end on the GPU.
 *
 * Stands where the reference's talker server computes, in numpy on the host, the text projection
 * `_embed_text` (gather text_embedding[ids] f32 [151936, 2048] -> fc1 + bias -> SiLU -> fc2 + bias -> [n, 1024])
 * and the dual-stream prefix `_build_prefix` (dual_npu/llamacpp_talker_server.py:115-161; tables loaded at
 * :79-93 from scripts/extract_embeddings.py:47-66's files).  Here the 1.24 GB f32 table lives in HBM as fp16
 * (0.62 GB), fc1 / fc2 are fp16 MFMA GEMMs with f32 accumulation (the talker's linear kernels; the biases are
 * the accumulators' initial values), SiLU and the prefix assembly are device kernels; the host hands over
 * token ids and receives the prefix rows it passes to wrapper_decode_embd / q3e_start.
 *
 * Numerics: the table and the two weight matrices are rounded to fp16 and the fc1 output after SiLU is a
 * fp16 GEMM input, everything else is f32: results agree with the reference's f32 arithmetic to ~1e-3 relative
 * (tests/test_gpu_text.py states the tolerance).  Prefix layout (rows): 3 role tokens (text only), tts_pad +
 * codec{nothink, think_bos, think_eos}, tts_bos + codec_pad, n x (text + codec_pad), tts_eos + codec_pad,
 * tts_pad + codec_bos = n + 9 rows.
 *
 * Caller-owned host buffers, synchronous calls, one caller thread per handle, no CPU fallback.
 */
#ifndef QWEN3TTS_TEXT_H
#define QWEN3TTS_TEXT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* weights: Q3TTSW1 container (or the HF snapshot's model.safetensors) holding text.embedding, text.fc{1,2}.{weight,bias}
 * and talker.codec_embedding; embeddings_dir: the reference's own embeddings/ directory instead (may be NULL).
 * max_tokens: longest text accepted by one call.  The text dim and the projection's mid width must be 2048 or 3072, the hidden
 * size a multiple of 128.  NULL on failure (message on stderr). */
void* tfe_load(const char* weights, const char* embeddings_dir, int max_tokens);
void tfe_free(void* h);
int tfe_hidden_size(void* h);      /* 1024 */
int tfe_text_vocab(void* h);

/* _embed_text: n token ids -> out[n][hidden] f32.  0 ok / <0 error (id out of range, n > max_tokens + 6). */
int tfe_embed_text(void* h, const int32_t* token_ids, int n, float* out);

/* _build_prefix: n text token ids (n >= 0) -> out[(n + 9)][hidden]; returns the number of rows, <0 on error.
 * `special` = the 12 ids {im_start, assistant, newline, tts_pad, tts_bos, tts_eos, codec_pad, codec_bos,
 * codec_nothink, codec_think_bos, codec_think_eos, 0} (llamacpp_talker_server.py:44-55,132); NULL = the
 * container's meta / the 0.6B defaults.  A text id outside the text table, or a codec id that is neither -1 (no codec
 * row added) nor inside the codec table, is an error; the handle stays usable. */
int tfe_build_prefix(void* h, const int32_t* text_token_ids, int n, const int32_t* special, float* out);

/* The projected tts_pad row (tts_client.py:58-69 computes it once; q3e_set_pad_embed takes it). */
int tfe_tts_pad_embed(void* h, float* out /*[hidden]*/);

/* Text streamed into a running utterance (q3e_push_text, qwen3tts_engine.h).  The streaming prefix needs only the first
 * text token: rows 0..6 of tfe_build_prefix (3 role rows, tts_pad + codec{nothink, think_bos, think_eos}, tts_bos +
 * codec_pad), then first token + codec_bos = 8 rows; returns 8, <0 on error.  `special` as for tfe_build_prefix.  The
 * rows that follow frame by frame are tfe_embed_text of tokens 1.. and, last, the projected tts_eos row.  This layout is
 * a recollection of the model's streaming mode (the reference implements only the non-streaming one and names the gap,
 * tts_client.py:56): same rows as the non-streaming prefix with the text moved out of it; parity with the model's own
 * streaming mode on real weights is not pinned. */
int tfe_build_prefix_stream(void* h, int32_t first_token_id, const int32_t* special, float* out /*[8][hidden]*/);
int tfe_tts_eos_embed(void* h, float* out /*[hidden]*/);

/* The same prefixes with a speaker embedding (qwen3tts_spk.h, spk_embed; spk_dim() must equal the hidden size): ONE row
 * inserted after the tts_pad + codec_think_eos row (index 5), tts_pad_embed + spk, an f32 add in that order -> n + 10 rows
 * (stream: 9); every other row is the row of the function above.  spk == NULL is exactly the function above.  <0 also for a
 * non-finite spk value.  The row's position is a recollection of the model's voice-clone prefix (qwen_tts is not importable
 * here), not pinned. */
int tfe_build_prefix_spk(void* h, const int32_t* text_token_ids, int n, const int32_t* special, const float* spk /*[hidden]*/,
                         float* out);
int tfe_build_prefix_stream_spk(void* h, int32_t first_token_id, const int32_t* special, const float* spk /*[hidden]*/,
                                float* out /*[9][hidden]*/);

#ifdef __cplusplus
}
#endif
#endif /* QWEN3TTS_TEXT_H */
