/*
 * qwen3tts_engine.h -- C ABI of the fused on-device frame loop (batch mode).
 *
 * Not present in the reference: there the autoregressive loop is closed by the Python client
 * over two sockets per frame (dual_npu/tts_client.py:144-215): talker hidden + code_0
 * (llamacpp_talker_server.py:254-293) -> code predictor (code_predictor_server.py:94-140)
 * -> feedback embedding (tts_client.py:199-208) -> next talker step.  This library keeps that
 * whole cycle on the GPU for B independent utterances: per frame one
 * hipGraph launch; the host only reads the codec ids.  Greedy decoding (the reference's
 * --temperature 0 limit); EOS rule, EOS boost, repetition penalty and the 2048..2149 / >=2151
 * mask are those of llamacpp_talker_server.py:163-206,258.
 *
 * Caller-owned host buffers, synchronous calls, one caller thread per handle, no CPU fallback.
 */
#ifndef QWEN3TTS_ENGINE_H
#define QWEN3TTS_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Number of visible HIP devices (0 = none: every loader of this library then returns NULL; there is no
 * CPU path), and selection of the device used by handles created afterwards (one process per GPU:
 * the per-GPU launcher sets HIP_VISIBLE_DEVICES, a torchrun rank passes LOCAL_RANK). */
int q3_device_count(void);
int q3_device_compute_units(void);   /* compute units of the current device (256 on an MI355X) */
int q3_set_device(int device);

/* weights: Q3TTSW1 container with talker.* and cp.*.  max_batch utterances at once, n_ctx talker
 * positions per utterance (prefix + frames), max_frames frames kept per utterance. */
void* q3e_create(const char* weights, int max_batch, int n_ctx, int max_frames);
void q3e_free(void* e);

/* Sampling.  Defaults are greedy (temperature 0 = the reference's --temperature 0 limit).  With
 * temperature > 1e-6 the device draws from top-k / temperature (/ top-p for the talker) like
 * llamacpp_talker_server.py:191-206 and code_predictor_server.py:87-92; the generator is counter based
 * (seed, request, utterance, frame, group): the first q3e_start after this call draws from `seed` itself,
 * every later one from a stream derived from (seed, request index), so a server replays nothing across
 * requests, a run is reproducible for a seed, and nothing is bit-compatible with numpy's or mt19937's streams.
 * top_k <= 0 (or >= the vocabulary) keeps every entry, as in the reference. */
int q3e_set_sampling(void* e, float talker_temperature, int talker_top_k, float talker_top_p,
                     float cp_temperature, int cp_top_k, uint64_t seed);

/* Teacher forcing: forced[f][b][16] (f < n_frames, b < B of the batch just started; entries < 0 = free-running).
 * Every decision the device takes is still recorded in the codes array, but the ids that are FED BACK (the
 * repetition window, the code predictor's inputs, the feedback embedding) are the forced ones -- continuing a
 * given codec prompt, and what the parity tests use to grade every decision of a run against the oracle, not only
 * those before the first near-tie.  Call after q3e_start; NULL switches it off; the next q3e_start resets it. */
int q3e_set_forced_codes(void* e, const int32_t* forced, int n_frames);

/* Split every frame step into n (1..8) independent row groups that run as parallel branches of the
 * captured graph: hides per-kernel launch latency behind the other groups' work at the price of
 * streaming the weights n times.  Default 1 (env Q3_CHAINS overrides): on ROCm 7.2 the
 * per-chain graphs were measured NOT to overlap, so more chains only re-stream the weights.
 * One chain runs on the engine's own stream; the per-chain streams and events are created by the first
 * call (or Q3_CHAINS) that asks for more than one, so the default engine holds one hardware queue.
 * Any chain count gives the same codes, and it may change between two q3e_run calls of a running batch. */
int q3e_set_chains(void* e, int n);

/* tts_pad embedding added to every feedback (tts_client.py:207-208); zeros until set. */
int q3e_set_pad_embed(void* e, const float* pad_embed /*[hidden]*/);

/* Begin a batch of B utterances.  prefix: the dual-stream prefix rows of all utterances,
 * concatenated ([sum n_rows][hidden] f32, llamacpp_talker_server.py:121-161); n_rows[b] rows
 * belong to utterance b; n_text[b] = number of text tokens (EOS heuristics, :172-181).
 * ignore_eos != 0 suppresses EOS (fixed-length benchmarking); max_frames caps every utterance
 * (the server's --max_tokens).  Runs the prefill; 0 ok / <0 error. */
int q3e_start(void* e, int B, const float* prefix, const int32_t* n_rows, const int32_t* n_text,
              int ignore_eos, int max_frames);

/* Generate up to n_frames more frames for the whole batch (returns early once every utterance
 * has finished; never steps past the max_frames given to q3e_start: 0 when none is left; in a per-slot
 * batch never past the text rows a live text slot has, see q3e_push_text).  Returns the number of frame
 * steps executed, <0 on error. */
int q3e_run(void* e, int n_frames);

/* Nodes of the captured frame (the first chain's graph): 0 before the first capture, <0 on error.  Between a call that
 * changes what the frame takes and the q3e_run that captures again it still reports the last capture.  A diagnostic: the
 * count is the same with and without q3e_scores_reserve. */
int q3e_graph_nodes(void* e);

/* GPU time of the last q3e_run / q3e_start in milliseconds (HIP events on the engine's stream). */
float q3e_last_run_ms(void* e);
float q3e_last_prefill_ms(void* e);

/* Codes so far: out[f][b][16] for f < returned frame count (<= max_out_frames); rows of finished
 * utterances hold -1 in column 0.  n_frames_per_utt[b] = frames utterance b really emitted. */
int q3e_get_codes(void* e, int32_t* out, int max_out_frames, int32_t* n_frames_per_utt);

/* Log-probabilities of the emitted ids (opt-in; DESIGN.md 2 "The score of an emitted id").
 *
 * For each of a frame's 16 sampling decisions the device records one f32: the model's log-probability, at temperature 1, of
 * THE ID THE STREAM CONTINUES WITH -- the id that is fed back: the forced one where q3e_set_forced_codes replaces the
 * decision, else the chosen one.  With z = the raw logit (NaN read as +inf) and m the maximum over the set,
 *     lp = z_u - m - log(sum_v exp(z_v - m)),
 * for column 0 over the talker's allowed set {v < cp_vocab} + {codec_eos} (an id outside it scores -inf), for columns 1..15
 * over all cp_vocab logits of the group's head.  It is the model's distribution, not the sampler's: temperature, top-k /
 * top-p, the repetition penalty, the EOS boost and masks, ignore_eos, forcing and the per-slot rules leave it unchanged.
 * Degenerate rows give the IEEE result of the formula (m = +inf, or nothing above -inf: NaN; a -inf id beside finite ones:
 * -inf).  fp32, expf / logf, one fixed reduction order: the same bits run to run.
 *
 * q3e_scores_reserve(e, 1): allocates the scores [max_frames][max_batch][16] (laid out like the codes) and makes the pointer
 * an argument of the frame's 16 sampling launches, which are then kernels of their own (*_scores); the next q3e_run
 * captures again.  No launch and no graph node is added.  0 releases.  <0 with nothing changed while a per-slot batch is
 * open (call before q3e_open, like q3e_rules_reserve).  An engine that never calls it launches the kernels it always did,
 * and with or without it the codes are the same bits in every mode.  A slot's scores are zeroed wherever its codes are reset.
 *
 * q3e_get_scores: out[f][b][16], the frame count and n_frames_per_utt of q3e_get_codes.  Every entry of a frame whose
 * column 0 of the codes is < 0, and of a frame at or past the utterance's count, reads 0.0f.  <0 without a reservation. */
int q3e_scores_reserve(void* e, int on);
int q3e_get_scores(void* e, float* out, int max_out_frames, int32_t* n_frames_per_utt);

/* Continuous batching (no counterpart in the reference, whose servers take one request at a time: SURVEY.md 8f2).
 * q3e_get_done: done[b] = 1 once utterance b has ended (EOS, or its frame budget); frames[b] (may be NULL) = frames it
 * has emitted.  q3e_refill: put n NEW utterances into the given slots of the running batch (finished or not) without
 * touching the others: the slots' counters, token history and codes column restart, their prefixes are prefilled
 * (prefix / n_rows / n_text as for q3e_start, in the order of `slots`), and the next q3e_run continues every slot --
 * the new ones with the full max_frames budget of q3e_start.  Fetch a finished utterance's codes (q3e_get_codes) BEFORE
 * refilling its slot.  After a refill q3e_get_codes returns rows up to the longest-running slot's frame count; each
 * column b holds utterance b's frames from ITS start (row f = its f-th frame).  0 ok / <0 error. */
int q3e_get_done(void* e, int32_t* done /*[B]*/, int32_t* frames /*[B] or NULL*/);
int q3e_refill(void* e, int n, const int32_t* slots, const float* prefix, const int32_t* n_rows, const int32_t* n_text);

/* Per-slot mode: utterances of different requests in one running frame loop.
 *
 * q3e_open: begin a batch of B slots that are all idle (ended, no frame, no prefix).  Idle slots still step through
 * the captured frame with the others, on zeroed caches and activations.  Every row then reads its own frame budget,
 * sampling settings and draw stream from a device array (one entry per slot), and the frame's dynamic LDS is sized for
 * the sampler's sort path, so admitting an utterance never recaptures the graph.  ignore_eos as for q3e_start.
 *
 * q3e_admit: put n new utterances into the given slots (as q3e_refill: the slots' counters, token history and codes
 * column restart; prefix / n_rows / n_text as for q3e_start, in the order of `slots`), each with its parameter block.
 * Every utterance is prefilled in a pass of its own, so its prefix sums do not depend on what is admitted beside it.
 * Requires 1 <= max_frames <= the max_frames of q3e_create and n_rows + max_frames <= n_ctx per utterance, finite
 * temperatures >= 0 and top_p in (0, 1].
 *
 * Seed contract: the utterance with index `utt` of a request with seed s draws from the stream mix(s, utt), mix = the
 * splitmix64 step (z = s + 0x9E3779B97F4A7C15 * (utt + 1), then the splitmix64 finaliser); every draw is keyed by
 * (stream, frame, group) -- group 0 the talker, 1 + g the code predictor's group g -- and NOT by the slot.  The same
 * utterance with the same seed therefore samples the same codes in any slot, beside any other utterances, after any
 * number of earlier admissions.  (q3e_start / q3e_refill keep their own derivation, with the row in the key.)
 *
 * q3e_release: mark n slots ended (cancellation); their rows go idle at the next step.
 *
 * A per-slot batch may step for the life of a server: no device or host counter grows with the number of steps (an ended
 * row's frame counter stops just past the codes array).
 *
 * In this mode q3e_get_done reports an utterance as ended once it has emitted its own budget, q3e_run never steps
 * past the largest budget a live slot has left and returns early once every admitted utterance has ended, and
 * q3e_get_codes returns rows up to the frame count of the slot admitted longest ago (column b = slot b's utterance
 * from its own start).  q3e_refill and q3e_set_forced_codes refuse a per-slot batch; q3e_start leaves the mode.
 * 0 ok / <0 error. */
typedef struct q3e_slot_params {
    int32_t max_frames;     /* frame budget of the utterance (the server's per-request max_tokens) */
    float temperature;      /* talker: <= 1e-6 arg-max, else top-k / temperature / top-p draws */
    int32_t top_k;          /* <= 0 or >= the vocabulary: every entry */
    float top_p;            /* (0, 1]; 1 keeps every entry */
    float cp_temperature;   /* code predictor: temperature and top-k */
    int32_t cp_top_k;
    uint64_t seed;          /* the request's seed ... */
    int32_t utt;            /* ... and the utterance's index in its request: the draw stream is mix(seed, utt) */
    int32_t reserved;       /* bit 0: a text slot (below); bit 1, valid only with bit 0: a text slot that may continue a codec
                             * prompt (q3e_admit_prompted); the other bits 0 */
} q3e_slot_params;

int q3e_open(void* e, int B, int ignore_eos);
int q3e_admit(void* e, int n, const int32_t* slots, const float* prefix, const int32_t* n_rows, const int32_t* n_text,
              const q3e_slot_params* params);
int q3e_release(void* e, int n, const int32_t* slots);

/* Prefix cache of the per-slot admissions (the reference's KV prefix cache, llamacpp_talker_server.py:208-246: md5 of the
 * prefix -> saved KV state + last hidden, a hit skips the prefill -- here for q3e_admit, on the device).
 *
 * q3e_admit prefills every utterance in a pass of its own, so the KV rows and the frame-0 state it leaves depend on the
 * prefix rows and on nothing else: not the slot, not the neighbours, not B.  An entry holds a copy of them -- rows
 * [0, n_rows) of K and V of every talker layer and KV head, and the last row's pre-norm residual with its sum-of-squares
 * partials.  A hit copies the rows into the slot in ONE launch over all layers and runs the final norm a prefill runs on
 * the saved residual, so the slot holds, bit for bit, what a prefill would have written: a reply with the cache is the
 * reply without it.  Everything is ordered on the engine's one stream; the cache adds no stream, event or hardware queue.
 *
 * q3e_prefix_cache: reserve (n_entries > 0) or release (0) a device pool of prefix entries, each up to max_rows rows
 * (clamped to the n_ctx of q3e_create).  Drops every entry; the counters of q3e_prefix_stats run on.  Not part of the
 * captured frame: legal at any time between calls, never recaptures.  <0 = nothing changed (negative arguments, entries
 * of 0 rows, no memory).  Pool size: n_entries * max_rows * (layers * 2 * n_kv * 128 * 2) bytes -- 114 688 B per row on
 * the 28-layer model (n_kv 8), 7.3 MB for an entry of 64 rows -- plus (hidden + hidden / 16) * 4 bytes per entry.
 * Entries survive q3e_open, q3e_set_chains and q3e_text_reserve (none changes what a prefill computes); q3e_free frees
 * the pool.
 *
 * q3e_admit_keyed: q3e_admit with a 128-bit key per utterance (keys[2 * u], keys[2 * u + 1]; {0, 0} or keys == NULL:
 * not cached, exactly q3e_admit).  Rows are always given.  Validation is q3e_admit's, before anything changes: a failed
 * call leaves the slots and the cache as they were.  Utterances are processed in order (a key given twice in one call is
 * a miss followed by a hit):
 *   - hit (the key is present with the same n_rows): the rows are neither uploaded nor read; the slot's KV rows and
 *     frame-0 state come from the entry;
 *   - miss: prefill as q3e_admit, then store under the key, into a free entry or over the least recently used one (use =
 *     hit or store).  A key present with another n_rows is a miss that replaces that entry.  Without a pool a keyed
 *     utterance is a miss that stores nothing;
 *   - n_rows > max_rows of the pool: a plain admission, counted as too long (neither hit nor miss).
 * hit[u] (may be NULL) = 1 / 0.  Text slots (`reserved` bit 0) may be keyed like any other: the entry holds the prefix,
 * not the pushed rows.  q3e_last_prefill_ms covers the call, as for q3e_admit.
 *
 * The key contract is the caller's: a key is a digest of EVERYTHING that determines the prefix rows (the token ids, the
 * kind of prefix, the model if handles share keys); the engine never compares rows.  Only the per-slot mode uses the
 * cache: q3e_start and q3e_refill prefill in shared passes whose sums are not a function of one prefix alone.
 *
 * q3e_prefix_stats: out[6] = hits, misses, stores, evictions, too long to cache, entries in use.  0 ok / <0 error. */
int q3e_prefix_cache(void* e, int n_entries, int max_rows);
int q3e_admit_keyed(void* e, int n, const int32_t* slots, const float* prefix, const int32_t* n_rows, const int32_t* n_text,
                    const q3e_slot_params* params, const uint64_t* keys, int32_t* hit);
int q3e_prefix_stats(void* e, int64_t* out /*[6]*/);

/* Codec prompts of the per-slot admissions: an utterance that continues given audio (the ids qwen3tts_enc.h makes of a
 * reference clip).  Not present in the reference.  What text the prefix holds beside the prompt is the caller's choice;
 * parity with the real model's prompted mode on real weights is NOT pinned, the arithmetic is: tests grade every frame
 * against the CPU oracle fed the same rows and the same history.
 *
 * q3e_admit_prompted: q3e_admit_keyed where utterance u may carry T = prompt_frames[u] frames of 16 codec ids
 * (prompt_codes: [sum T][16], in the order of the utterances) that count as frames it has ALREADY emitted:
 *   - rows: prompt frame i is talker row n_rows + i, = codec_embedding[P[i][0]] + sum over g = 0..14 of
 *     cp_table[g][P[i][1 + g]] + tts_pad (what q3e_set_pad_embed last set), added in that order in f32: the feedback sum
 *     of tts_client.py:199-208, built on the device by the frame loop's own code.  The utterance's pass prefills n_rows + T
 *     rows, and the slot's KV rows and frame-0 state are, bit for bit, what q3e_admit leaves when given the n_rows + T rows
 *     [prefix ; rows(P)] as a plain prefix;
 *   - sampler state: the emitted-token ring holds P[i][0] for the last min(T, 32) frames and the utterance has T frames
 *     behind it: the repetition window (the last 30), the EOS-boost progress (T + frames generated) / (3 * n_text) and the
 *     forced EOS above 2.0 of llamacpp_talker_server.py:163-206 all see the prompt;
 *   - generated frames: the codes array, q3e_get_done, q3e_get_codes and the budget count GENERATED frames only: row 0 of
 *     the slot's column is its first generated frame, `max_frames` of q3e_slot_params is the number of generated frames,
 *     and the draw key stays (stream, generated frame index, group), so the seed contract above holds unchanged;
 *   - positions: the first frame step runs at position n_rows + T.
 * Validation is q3e_admit's, before anything changes, with n_rows + T where it has n_rows (the rows one prefill pass
 * takes, and n_rows + T + max_frames <= n_ctx), and: T >= 0, column 0 of every prompt frame in 0..2047 (an audio id),
 * columns 1..15 inside the code predictor's vocabulary, no prompt on a text slot that did not ask for one (`reserved`
 * == 1; == 3 below).  A failed call leaves the slots and the cache as they were.  prompt_frames == NULL, or T = 0 for an
 * utterance: exactly q3e_admit_keyed.
 *
 * Text slots that continue a prompt (streamed text in a cloned voice): `reserved` == 3 (bits 0 and 1) admits a text slot
 * WITH its T prompt frames; == 2 is refused, == 3 without q3e_text_reserve is refused like any text slot, == 3 with T = 0
 * is exactly == 1.  Rows, KV, frame-0 state, ring, positions, validation and the cache are those of an ordinary prompted
 * slot (the prompt's rows add tts_pad), and the slot's text is counted by the GENERATED frame: pushed row i is row i of
 * the slot's reservation and stands where tts_pad would in the feedback of generated frame i -- the frame row i of the
 * slot's column of the codes array holds -- so the reservation keeps its size (rows <= max_frames) and q3e_push_text,
 * q3e_text_state, q3e_text_held, q3e_get_done, q3e_get_codes and q3e_release keep their contracts.  Starved, stalled and
 * held (q3e_text_hold) are judged with g = the frames generated: held when g >= 1 and g >= the rows pushed, a stall of
 * the batch at g == 0 without a row.  EOS is masked until the final push; from then on n_text = n_text_total and the
 * rules see T + g emitted frames, as for an ordinary prompted slot.  The layout (a streaming prefix, then the prompt, then
 * text rows riding on the generated frames) is, like both of its halves, a recollection: parity on real weights is NOT
 * pinned, the arithmetic is.
 *
 * Prefix cache: an entry of a prompted utterance holds its n_rows + T rows and the last prompt row's residual state, and
 * n_rows + T is the length the index compares (and compares with the pool's max_rows: a longer utterance is a plain
 * admission, counted as too long).  On a hit the prefix rows are not read; the prompt codes always are, the ring is
 * rebuilt from them.  The key contract stays the caller's: the digest must cover the prompt.
 *
 * The prompt costs one launch per prompted utterance on the engine's stream, outside the captured frame, which does not
 * change: no recapture, no new stream, event or hardware queue.  0 ok / <0 error. */
int q3e_admit_prompted(void* e, int n, const int32_t* slots, const float* prefix, const int32_t* n_rows, const int32_t* n_text,
                       const q3e_slot_params* params, const uint64_t* keys, int32_t* hit,
                       const int32_t* prompt_codes /* [sum T][16], utterance order */,
                       const int32_t* prompt_frames /* [n], 0 = none */);

/* Sampler rules per slot (per-slot mode only).  Contract: every rule of the talker sampler that is a constant of
 * llamacpp_talker_server.py:163-206 -- the repetition penalty 1.2 over the last 30 ids, the adaptive EOS boost of up to 15
 * from 0.8 of the expected length, the forced EOS above 2.0 of it, no minimum length -- and the code predictor's missing
 * nucleus cut become values of the slot.  The defaults ARE those constants (the penalty the same f32 1.2f, the others exact
 * in f32): a slot with default rules, an admission without rules and an engine without a reservation give the same codes,
 * bit for bit.
 *   rep_penalty  finite, >= 1.  A penalised logit l becomes l / p when l > 0, else l * p (the reference's operations); 1
 *                changes nothing, exactly.
 *   rep_window   1..30: the ids penalised are the last min(emitted, w) of the utterance, a codec prompt's frames included.
 *                0: EVERY id the utterance has emitted, prompt frames included -- the semantics of transformers'
 *                RepetitionPenaltyLogitsProcessor over the emitted ids.  The engine keeps a set of emitted ids per slot
 *                (one bit per audio id) for it; ids outside the audio vocabulary have no bit and are never emitted.
 *   eos_boost    finite, >= 0: the boost is (float)(b * (double)eos_boost), b = min((progress - 0.8) / 0.7, 1) in double
 *                as in the reference (0.8 and 0.7 stay constants); 0 adds nothing.
 *   eos_force    finite, >= 0: EOS replaces the decision when progress > eos_force; 0 never forces.
 *   min_frames   >= 0: until the utterance has GENERATED this many frames its EOS logit is -1e10 (as under ignore_eos):
 *                no boost, and a forced EOS is not applied.  The budget still ends the utterance.
 *   cp_top_p     (0, 1]: nucleus cut of the code predictor's stochastic draws, by the talker's rule (the smallest prefix
 *                of the descending order whose mass reaches it); 1 = none; arg-max ignores it.
 *   reserved     0.
 * progress = (prompt frames + frames generated) / (3 * n_text) as before; a text slot's EOS mask and min_frames both put
 * EOS at -1e10 and compose.
 *
 * q3e_default_rules: the defaults above into *out.
 *
 * q3e_rules_reserve(e, 1): call before q3e_open.  Allocates the rules entry and the emitted-id set of max_batch slots (24 +
 * 256 bytes per slot at an audio vocabulary of 2048) and makes their pointers arguments of the captured frame, so the next
 * q3e_run captures again and admitting a ruled utterance never does; 0 releases them.  <0 with nothing changed while a
 * per-slot batch is open.  An engine that never calls it captures the frame it always did and launches the kernels it
 * always did.
 *
 * q3e_admit_ruled: q3e_admit_prompted with a rules block per utterance.  rules == NULL, or a block equal to the defaults,
 * is exactly q3e_admit_prompted; non-NULL rules without a reservation are refused.  Validation (the ranges above,
 * non-finite values, reserved != 0, min_frames < 0) comes with q3e_admit's, before anything changes: a failed call leaves
 * the slots, the cache and the emitted-id sets as they were.  Under a reservation every admission starts its slot with an
 * empty set (then the prompt's ids) and default rules unless it brings its own: a recycled slot inherits nothing.  Rules do
 * not enter what a prefill computes: the prefix cache and its key contract are untouched.  q3e_start / q3e_refill /
 * q3e_set_sampling keep the constants.  0 ok / <0 error. */
typedef struct q3e_slot_rules {
    float rep_penalty;   /* >= 1, 1 = none            (reference: 1.2) */
    int32_t rep_window;  /* 1..30 last ids, 0 = whole utterance (30)   */
    float eos_boost;     /* >= 0, ceiling of the adaptive boost (15)   */
    float eos_force;     /* progress above which EOS is forced, 0 = never (2) */
    int32_t min_frames;  /* GENERATED frames before EOS may be chosen (0) */
    float cp_top_p;      /* (0, 1], 1 = none (1) */
    int32_t reserved[2]; /* 0 */
} q3e_slot_rules;
void q3e_default_rules(q3e_slot_rules* out);
int q3e_rules_reserve(void* e, int on);
int q3e_admit_ruled(void* e, int n, const int32_t* slots, const float* prefix, const int32_t* n_rows, const int32_t* n_text,
                    const q3e_slot_params* params, const uint64_t* keys, int32_t* hit, const int32_t* prompt_codes,
                    const int32_t* prompt_frames, const q3e_slot_rules* rules /* [n], or NULL */);

/* Text streamed into a running utterance, row by row (per-slot mode only).
 *
 * Layout (a recollection of the model's streaming mode, which the reference does not implement -- it pre-computes the
 * pad row "for non-streaming feedback", tts_client.py:56; parity with the real model on real weights is NOT pinned, the
 * arithmetic is: tests grade every frame against the CPU oracle fed the same rows): the prefix holds only the first text
 * token (tfe_build_prefix_stream, 8 rows), and the feedback of frame f of the slot (f from its own start) adds, where
 * tts_client.py:207-208 adds tts_pad, row f of the slot's text rows R = [T[1], .., T[n-1], E] (T = tfe_embed_text of the
 * ids, E = tfe_tts_eos_embed) while f < n, and the pad row afterwards.
 *
 * q3e_text_reserve: call before q3e_open.  Allocates [max_batch][max_rows][hidden] f32 and the per-slot row counters
 * (32 MiB at 32 x 256 x 1024); max_rows <= the max_frames of q3e_create (a row past the budget could never be
 * consumed); 0 releases the reservation.  The pointers are part of the captured frame, so they are fixed here and
 * admitting a text slot never recaptures; an engine that never calls this captures the frame it always did.  Refused
 * while a text slot is live.
 *
 * A q3e_slot_params with bit 0 of `reserved` set admits a text slot: q3e_admit refuses it (<0, nothing changed) without
 * a reservation; its n_text is ignored; prefix / n_rows are the streaming prefix, or any rows the caller likes.
 *
 * q3e_push_text: append n >= 0 rows ([n][hidden] f32) to the slot's text.  final != 0 ends the text.  Until then the
 * slot's EOS logit is masked (as under ignore_eos) and its n_text is 0 (no boost, no forced EOS); the final push lifts
 * the mask and sets n_text to n_text_total, so from the next sampled frame on the rules of
 * llamacpp_talker_server.py:167-181 apply unchanged (a batch-wide ignore_eos still masks EOS for every slot).
 * <0 with nothing written (the call can be retried): the slot is not a live text slot, a push after the final one,
 * rows beyond the reservation, a non-finite value.
 *
 * A slot never runs ahead of its text: row i is always consumed at frame i, so a slot's codes depend on its text and on
 * nothing about arrival times.  What a live text slot WITHOUT a row for its next frame (a starved slot) does to the
 * others depends on the mode:
 *   - default: it stalls the WHOLE batch.  q3e_run executes no step whose frame has no row yet -- it runs the steps every
 *     such slot has rows for and returns their number, which may be 0; the host decides whether to wait, push, or
 *     release the slot.
 *   - q3e_text_hold(e, 1), called between q3e_text_reserve and q3e_open (<0 with nothing changed without a reservation
 *     or while a per-slot batch is open; it changes arguments of the captured frame, so the next q3e_run captures
 *     again): the starved slot is HELD inside the frame and the others step on.  The sampler leaves a held row's
 *     counters, codes and logits alone, the code predictor continues with the ids the row's last frame records, and the
 *     rest of the frame thereby recomputes the row's previous step onto itself: after the step the row's state is, bit
 *     for bit, what it was before, and the other rows never depended on it.  q3e_run then executes min(n_frames, the
 *     most steps a live slot can still use) steps: up to its rows for a text slot before its final push, up to its
 *     budget for any other; 0 only when every live slot is held -- or when some live text slot has no frame yet and
 *     no row (nothing of its own to repeat: such a slot still stalls the batch, so admit a text slot with its first
 *     row at hand).  Slots then differ in the frames they have emitted by the steps they were held for; q3e_get_done,
 *     q3e_get_codes and q3e_release keep their contracts with those per-slot counts.  A push lifts the hold from the
 *     next step on (a final push with n = 0 as well: the slot goes on with pad rows), releasing a held slot ends it, and
 *     a slot at its budget is never held, so it ends there.
 *
 * q3e_text_state: rows[b] = rows pushed to slot b (0: not a text slot), starved[b] = 1 when slot b is a live text slot
 * the next step waits for (in either mode).  Either pointer may be NULL.  q3e_text_held: held_steps[b] = frame steps
 * slot b's utterance was held for since its admission (0 without q3e_text_hold).  0 ok / <0 error. */
int q3e_text_reserve(void* e, int max_rows);
int q3e_text_hold(void* e, int on);
int q3e_text_held(void* e, int64_t* held_steps /*[B]*/);
int q3e_push_text(void* e, int slot, const float* rows, int n, int final, int n_text_total);
int q3e_text_state(void* e, int32_t* rows /*[B]*/, int32_t* starved /*[B]*/);

/* Talker hidden state of every utterance after the last executed step ([B][hidden]). */
int q3e_get_hidden(void* e, float* out);

/* Algorithmic weight bytes one frame step streams (talker stack + head + 16 CP passes + 15 heads).  With the code
 * predictor's layer-0 q|k|v table (the default; Q3_CP_QKV_TABLE=0 at load turns it off and saves its 470 MB of device
 * memory) 14 of those passes read one 16 KB table row per utterance instead of layer 0's q|k|v weights. */
double q3e_step_weight_bytes(void* e);

#ifdef __cplusplus
}
#endif
#endif /* QWEN3TTS_ENGINE_H */
