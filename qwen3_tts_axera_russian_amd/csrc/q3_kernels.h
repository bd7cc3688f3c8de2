// q3_kernels.h -- launch interface of the gfx950 kernels (q3_linear.hip, q3_attn.hip, q3_sample.hip, q3_rows.hip).
//
// Numerics contract shared with oracle/q3_oracle.c (DESIGN.md "Numerics"):
//   * projection weights fp16, residual stream / norms / softmax / tables f32,
//     every GEMM input rounded to fp16 (saturating), f32 accumulation;
//   * RMSNorm folded around the GEMM: input xh = fp16((h*gamma)/16) written by the producer of h,
//     accumulators multiplied by inv_rms(row)*16;
//   * K/V cache fp16, q kept f32.
#pragma once
#include "q3_common.h"
#include "q3_frag.h"

namespace q3 {

enum { PRO_F16 = 0, PRO_NORM = 1 };
enum { EPI_STORE = 0, EPI_RESID = 1, EPI_SWIGLU = 2 };

// y[M][N] = A[M][K] . W[N][K]^T with W in MFMA-fragment order (see pack_linear).
struct LinArgs {
    int tl_node = -1;  // diagnostic timeline build only: graph node index
    const half_t* wp = nullptr;  // packed weights
    int N = 0, K = 0, M = 0;   // rows [m_begin, M) are computed
    int m_begin = 0;
    int swap_grid = 0;  // set by the launcher
    int nt = 0;  // 1: stream the weights with non-temporal loads (read once per step: talker)
    // A operands are stored in MFMA fragment order (frag_idx), buffers padded to 16 rows.
    // prologue PRO_F16: A = x16[M][K] (fp16).  PRO_NORM: A = x16 = the producer's xh = fp16((h*gamma)/16) and the
    // accumulators are multiplied by 16*inv[m], inv[m] = 1/sqrt(sum(ssq[m][0..ssq_parts))/K + eps).
    const half_t* x16 = nullptr;
    const float* ssq = nullptr;
    int ssq_parts = 0;
    float eps = 1e-6f;
    // EPI_STORE: y[m*ldy + n] = acc
    float* y = nullptr;
    int ldy = 0;
    // EPI_RESID: h_out[m*N+n] += acc; ssq_out[m*(N/16) + n/16] = sum of squares of the new 16 values;
    // xh_out[m][n] = fp16((h_out*gamma[n])/16) for the consumer whose norm weight is `gamma` (null: none)
    float* h_out = nullptr;
    float* ssq_out = nullptr;
    half_t* xh_out = nullptr;
    const float* gamma = nullptr;
    // EPI_SWIGLU (gate/up tile-interleaved weights): act[m*(N/2)+j] = fp16(silu(g)*u)
    half_t* act = nullptr;
};
int launch_linear(hipStream_t s, const LinArgs& a, int pro, int epi);
// How launch_linear's weight-streaming kernels would split K for `rows` rows of an N-column projection: k-blocks of 32 per
// wave (the waves' partial sums are added in wave order), or 0 where the rows go to the tiled GEMM / no kernel exists.
// Two row counts with the same answer add the products of one row in the same order: bit-identical rows.
int linear_decode_kbw(int K, int N, int rows);

// Repack a row-major fp16 matrix src[N][K] into fragment order inside dst:
// source 16-row tile ts lands at destination tile (tile_off + ts*tile_stride).
int launch_pack_linear(hipStream_t s, const half_t* src, int N, int K, half_t* dst, int tile_off,
                       int tile_stride);

enum { ATTN_FUSED = 0, ATTN_PREP = 1, ATTN_ATTEND = 2 };
struct AttnArgs {
    int tl_node = -1;  // diagnostic timeline build only: graph node index
    float* qkv = nullptr;  // [R][ld]: q heads, then k heads, then v heads (raw projections)
    int ld = 0, R = 0, row0 = 0;   // rows row0 .. row0+R-1
    const float* q_norm = nullptr;
    const float* k_norm = nullptr;
    float eps = 1e-6f;
    const float* rope_cos = nullptr;  // [max_pos][64]
    const float* rope_sin = nullptr;
    const int* slot = nullptr;  // [R] or null -> slot_base + r*slot_stride
    const int* pos = nullptr;   // [R] or null -> pos_base + r*pos_stride
    int slot_base = 0, slot_stride = 0, pos_base = 0, pos_stride = 0;
    half_t* kc = nullptr;  // this layer: [slot][n_kv][n_ctx][128]
    half_t* vc = nullptr;
    int n_ctx = 0, n_kv = 0, n_heads = 0;
    half_t* out = nullptr;  // [R][n_heads*128]
    float scale = 0.f;
    int threads = 256;
    // rows r with (r % valid_mod) >= valid_n are padding (no slot of their own): skipped.  0 = every row is real.
    int valid_mod = 0, valid_n = 0;
    // ATTN_ATTEND over runs of consecutive positions of one slot (prefill): tiles[i] = {first row, rows (1..16), slot,
    // position of the first row}; null with n_tiles > 0 = the rows row0.. are ONE run (slot_base, pos_base + i)
    const int* tiles = nullptr;
    int n_tiles = 0;
};
int launch_attn(hipStream_t s, const AttnArgs& a, int mode);

// Uploaded row-major rows[R][H] -> residual stream h in fragment order (see frag_idx in q3_frag.h)
// + ssq[m][p] = sum_{k in 16-block p} rows[m][k]^2  (H/16 partials per row)
// + xh = fp16((rows*gamma)/16), the pre-scaled GEMM input of the layer whose norm weight is gamma (null: none)
int launch_ssq_rows(hipStream_t s, const float* rows, float* h, float* ssq, int R, int H, half_t* xh = nullptr,
                    const float* gamma = nullptr, int dst_row0 = 0);   // input row r lands in row dst_row0 + r

// hidden = (h*inv)*gamma per row; optional outputs: f32 hidden, fp16 hidden,
// a second f32 copy (+ its ssq partials) that seeds the code predictor.
struct FinalNormArgs {
    int tl_node = -1;  // diagnostic timeline build only: graph node index
    const float* h = nullptr;
    const float* ssq = nullptr;
    int ssq_parts = 0;
    const float* gamma = nullptr;
    float eps = 1e-6f;
    int R = 0, H = 0, row0 = 0;    // output rows row0 .. row0+R-1
    const int* row_map = nullptr;  // optional: source row of output row r (indexed by the output row)
    int src_off = 0;               // without a map: source row = output row + src_off
    float* out_f32 = nullptr;
    half_t* out_f16 = nullptr;
    float* out_copy = nullptr;
    float* out_copy_ssq = nullptr;
    int out_copy_row_off = 0;                // the copy of output row r lands in row r + out_copy_row_off
    half_t* out_copy_xh = nullptr;           // pre-scaled GEMM input of the copy's consumer ...
    const float* out_copy_gamma = nullptr;   // ... whose norm weight this is
};
int launch_final_norm(hipStream_t s, const FinalNormArgs& a);

// h[r] = table[tok_r] (zeros when tok_r is out of range), with ssq partials.  tok_r = tok[r*tok_stride]
// when n_frames is null, else column `col` of row r's current frame in a codes array laid out as in
// TalkerSampleArgs (frame = n_frames[r]-1, clamped to [0, frame_cap)).
int launch_gather_embed(hipStream_t s, const float* table, int V, int H, const int* tok, int tok_stride,
                        const int* n_frames, int frame_cap, int col, float* h, float* ssq, int R, int row0 = 0,
                        int R_total = 0, const int* forced = nullptr, half_t* xh = nullptr, const float* gamma = nullptr);

// Prefix state of one utterance between its talker KV slot and a prefix-cache entry (q3e_admit_keyed), either way, in one
// launch over every layer: rows [0, n_rows) of K and V of every KV head -- one contiguous run of n_rows * 256 bytes per
// (layer, K|V, head) on both sides, moved 16 bytes per lane -- and the last prefix row's pre-norm residual with its
// sum-of-squares partials (what the final norm after a prefill reads), between row h_row of the fragment-ordered h / ssq
// and the entry's row-major state.
struct PrefixMoveArgs {
    half_t* kc = nullptr;       // talker cache: [layer][slot][n_kv][n_ctx][128]
    half_t* vc = nullptr;
    size_t layer_stride = 0;    // elements between two layers of kc / vc
    int n_layers = 0, n_kv = 0, n_ctx = 0;
    int slot = 0, n_rows = 0;   // n_rows <= min(n_ctx, max_rows)
    half_t* entry = nullptr;    // [layer][2][n_kv][max_rows][128]
    int max_rows = 0;
    float* state = nullptr;     // [H + H/16]: residual row, then its ssq partials
    float* h = nullptr;         // Work::h / Work::ssq of the talker
    float* ssq = nullptr;
    int h_row = 0, H = 0;
    int restore = 0;            // 0: slot -> entry, 1: entry -> slot
};
int launch_prefix_move(hipStream_t s, const PrefixMoveArgs& a);

// Per-slot parameters of the frame loop (q3e_open / q3e_admit): one entry per row of the batch.  When a sampling kernel
// gets a non-null `slots` array it reads the row's entry instead of its scalar fields (frame budget, temperature, top-k,
// top-p, draw seed); one workgroup handles one row, so every branch these values pick stays uniform in the workgroup.
struct SlotParams {
    int max_frames = 0;            // frame budget: the row ends once it has emitted this many frames
    float t_temp = 0.f;            // talker: temperature (<= 1e-6: arg-max), top-k, top-p
    int t_top_k = 0;
    float t_top_p = 1.f;
    float c_temp = 0.f;            // code predictor: temperature, top-k
    int c_top_k = 0;
    unsigned long long seed = 0;   // the row's draw stream
    int no_row = 1;                // 1: the draw key is (seed, frame, group), without the row index
    int flags = 0;                 // bit 0: a text slot (its feedback adds text_rows, see CpArgmaxArgs); bit 1: its EOS is masked
    int prompt = 0;                // codec-prompt frames n_past started at (q3e_admit_prompted): a text slot's hold test counts
                                   // the frames it generated, n_past - prompt (n_frames and the text rows already do)
};

// Per-slot sampler rules (q3e_rules_reserve / q3e_admit_ruled): one entry per row of the batch, in an array of its own
// beside SlotParams.  A sampling kernel given a non-null `rules` array reads the row's entry where it otherwise uses the
// constants of llamacpp_talker_server.py:163-206; the defaults below ARE those constants (the penalty the same f32, the
// others exact in f32), so a row with default rules gives the bits of a launch without the array.  Written by the host
// between launches only.
struct SlotRules {
    float rep_penalty = 1.2f;      // talker: finite, >= 1; replaces TalkerSampleArgs::rep_penalty for the row (1: none, exact)
    int rep_window = 30;           // 1..30: the last min(n_past, w) ids of the ring; 0: every id in the row's seen-set
    float eos_boost = 15.f;        // ceiling of the adaptive EOS boost, finite, >= 0 (0: nothing is added)
    float eos_force = 2.f;         // EOS is forced when progress > this; 0: never
    int min_past = 0;              // while n_past < min_past the EOS logit is -1e10f (as under ignore_eos) and no EOS is forced
    float cp_top_p = 1.f;          // code predictor: nucleus cut of the stochastic path, (0, 1]; 1: none
};

// Talker sampling (llamacpp_talker_server.py:163-206, greedy form).
struct TalkerSampleArgs {
    int tl_node = -1;  // diagnostic timeline build only: graph node index
    const float* logits = nullptr;  // [R][V]
    int V = 0, R = 0, row0 = 0, R_total = 0;   // rows row0..row0+R-1 of a batch of R_total (0 = R)
    int audio_vocab = 2048, eos = 2150;
    int* past = nullptr;    // [R][32] ring of emitted code_0
    int* n_past = nullptr;  // [R]
    const int* n_text = nullptr;  // [R]
    int* done = nullptr;          // [R]
    // codes of frame f of row r live at codes[(f*R + r)*16 .. +16); f = n_frames[r] (per-row counter,
    // incremented here; clamped to frame_cap-1).  Column 0 is written: code_0, or -1 once the row finished.
    int* codes = nullptr;
    int* n_frames = nullptr;      // [R]
    int frame_cap = 0;
    const int* pos0 = nullptr;    // [R] prefix length
    int* pos = nullptr;           // [R] position of the talker step that follows = pos0 + frames emitted before
    int ignore_eos = 0;
    int max_frames = 0;
    float rep_penalty = 1.2f;
    // temperature <= 1e-6: arg-max (the reference's limit); else top-k / temperature / top-p on the device
    float temperature = 0.f, top_p = 0.95f;
    int top_k = 50;              // <= 0 or >= V: every entry (the reference skips its argpartition then)
    unsigned long long seed = 0;
    const unsigned long long* seed_ptr = nullptr;  // device array [rows] overriding `seed`: one draw stream per slot (per request and per refill, graph-safe)
    // teacher forcing (tests): same layout as `codes`; entries >= 0 replace the decision that is FED BACK
    // (ring of past ids, CP input, feedback sum) while `codes` still records what the device decided
    const int* forced = nullptr;
    // per-slot mode (null: the scalar fields above): budget, temperature, top-k, top-p and draw key of row r come from
    // slots[r]; the dynamic LDS is then sized for the sort path whatever the row asks for
    const SlotParams* slots = nullptr;
    // per-slot mode with held text slots (q3e_text_hold; both null: none).  A row is HELD in this step when its slot is a
    // text slot whose text has not ended (flags 3), it has not ended, n_past < its budget, and with g = n_past -
    // slots[r].prompt, the frames it generated, g >= 1 and g >= text_avail[r]: its next frame has no text row yet, and it
    // has a frame of its own to repeat.  The workgroup of a held row sets held[r] and returns before it
    // reads a logit: no counter, code, ring entry or position of the row changes.  Every other row clears held[r].
    const int* text_avail = nullptr;    // [R_total] rows pushed per slot (written by the host between launches)
    int* held = nullptr;                // [R_total] 1: the row is held in this step (read by the frame's cp_argmax launches)
    // per-slot mode with sampler rules (q3e_rules_reserve; both null: the constants, and the kernel of a launch without
    // them).  rules[r] replaces rep_penalty, the window of 30, the boost of 15, the forced EOS above 2.0 and "no minimum"
    // for row r (SlotRules).  seen[r] is the row's set of emitted ids, one bit per audio id in (audio_vocab + 31) / 32
    // words: whenever it is given, the launch sets the bit of the id the stream continues with where it writes the ring
    // (ids outside [0, audio_vocab) have no bit), for every row whatever its window; a held row, an ended row and a row
    // outside the launch write nothing.  rep_window == 0 reads it, and so needs it.
    const SlotRules* rules = nullptr;   // [R_total]
    unsigned* seen = nullptr;           // [R_total][(audio_vocab + 31) / 32]
    // log-probabilities of the emitted ids (q3e_scores_reserve; null: none, and the kernels of a launch without them).  Laid
    // out like `codes`; column 0 of the row's frame gets the model's log-probability, at temperature 1, of the id the
    // stream continues with (the forced id where one replaces the decision): z_u - m - log(sum_A exp(z_v - m)) over the
    // allowed set A = {v < audio_vocab} + {eos} of the RAW logits (z = NaN read as +inf, m their maximum), -inf for an id
    // outside A.  No sampler setting enters it.  Written where column 0 of `codes` gets an id, nowhere else.
    float* scores = nullptr;
};
int launch_talker_sample(hipStream_t s, const TalkerSampleArgs& a);

// Code-predictor group argmax (+ next embedding gather, or the feedback sum
// of tts_client.py:199-208 after the last group).
struct CpArgmaxArgs {
    int tl_node = -1;  // diagnostic timeline build only: graph node index
    const float* logits = nullptr;  // [R][V]
    int V = 0, R = 0, H = 0, row0 = 0, R_total = 0;
    int group = 0;                 // writes column group+1 of the row's current frame
    int* codes = nullptr;          // as in TalkerSampleArgs (frame = n_frames[r]-1)
    const int* n_frames = nullptr;
    int frame_cap = 0;
    const float* next_table = nullptr;  // f32 [V][H] of this group, or null
    float* h_out = nullptr;
    float* ssq_out = nullptr;
    half_t* xh_out = nullptr;           // pre-scaled GEMM input for the layer that consumes h_out ...
    const float* gamma_next = nullptr;  // ... whose input norm weight this is
    // with next_table: row `token` of next_qkv (f32 [V][qkv_ld], Model::cp_qkv_tab of this group: layer 0's q|k|v of every
    // row of next_table) is copied into row r of qkv_out ([rows][qkv_ld], LinArgs::y / ldy of that launch); null = none
    const float* next_qkv = nullptr;
    float* qkv_out = nullptr;
    int qkv_ld = 0;
    // feedback (when talker_emb != null): h_out = talker_emb[code0] + sum_g cp_tables[g][code_{g+1}] + pad
    const float* talker_emb = nullptr;
    int talker_vocab = 0;
    const float* const* cp_tables = nullptr;  // device array [n_groups]
    const float* pad_embed = nullptr;
    int n_groups = 15;
    float temperature = 0.f;   // <= 1e-6: arg-max
    int top_k = 50;            // <= 0 or >= V: every entry
    unsigned long long seed = 0;
    const unsigned long long* seed_ptr = nullptr;  // device array [rows] overriding `seed` (one stream per slot)
    const int* forced = nullptr;                   // teacher forcing (tests), see TalkerSampleArgs
    const SlotParams* slots = nullptr;             // per-slot mode: temperature, top-k, draw key of row r (see TalkerSampleArgs)
    // (last, so that the fields above keep their kernarg offsets)
    // per-slot mode, text streamed into the utterance (q3e_text_reserve; null: none): the row added last to the feedback
    // of frame f of row r is text_rows[r][f] while f < text_avail[r] (<= text_cap), else pad_embed; f = n_frames[r] - 1 as the
    // slot counts it, NOT clamped to frame_cap (a row that ended past the codes array still adds its own frame's text row),
    // and a row without a frame yet (n_frames = 0) adds pad_embed.  Whether the slot is a text slot (flags) plays no part:
    // the host keeps text_avail 0 for the others.  Both arrays are written by the host between launches, never by a kernel
    // of the same launch.
    const float* text_rows = nullptr;   // f32 [R_total][text_cap][H]
    const int* text_avail = nullptr;    // [R_total]
    int text_cap = 0;
    // per-slot mode with held text slots (null: none): held[r] != 0 (set by this step's talker_sample launch) makes the
    // row continue with the id its current frame already records in this group's column, and store nothing: the gather,
    // the q|k|v copy and the feedback sum then repeat what they produced when that frame was first computed.
    const int* held = nullptr;          // [R_total]
    // per-slot mode with sampler rules (null: none): rules[r].cp_top_p is the nucleus cut of row r's stochastic draw
    // (block_sample_topk's top_p; without rules there is none).  The arg-max path ignores it.
    const SlotRules* rules = nullptr;   // [R_total]
    // log-probabilities of the emitted ids (see TalkerSampleArgs::scores; null: none): column group+1 of the row's frame
    // gets the log-softmax, over all V raw logits, of the id the stream continues with.  Written where that column of
    // `codes` is written: never for a held row (it keeps the score recorded with its id) or a frame beyond the array.
    float* scores = nullptr;
};
int launch_cp_argmax(hipStream_t s, const CpArgmaxArgs& a);

// Stand-alone feedback sum (tts_client.py:199-208) for host-provided codes.
int launch_feedback(hipStream_t s, const int* codes16, int R, const float* talker_emb, int talker_vocab,
                    const float* const* cp_tables, int cp_vocab, int n_groups, const float* pad_embed,
                    float* h_out, float* ssq_out, int H, half_t* xh_out = nullptr, const float* gamma = nullptr);

// Codec prompt of one admitted utterance (q3e_admit_prompted): T frames of 16 ids the utterance counts as already emitted.
// One launch, one workgroup per prompt frame i:
//   - with h != null, the frame's talker row -- the feedback sum of tts_client.py:199-208 (feedback_row, the frame loop's
//     own) -- goes to row row0 + i of the fragment-ordered h / ssq / xh, with the sum-of-squares partials and the pre-scaled
//     fp16 copy launch_ssq_rows gives a row of these values: the prefill reads it where it reads an uploaded row;
//   - the sampler's state of the slot: column 0 of the last min(T, 32) frames into the emitted-token ring at i & 31, and
//     n_past = T; with seen != null, the bit of column 0 of EVERY frame into the slot's seen-set (TalkerSampleArgs::seen;
//     the caller has cleared it): the workgroups share words, so each sets its bit with a vector atomic OR.
// The caller has checked the ids (column 0 < talker_vocab, the others < cp_vocab, none negative) and row0 + T <= max_rows.
struct PromptRowsArgs {
    const int* codes = nullptr;   // device [T][16]
    int T = 0;
    int* past = nullptr;          // the slot's ring [32]
    int* n_past = nullptr;        // the slot's counter
    unsigned* seen = nullptr;     // the slot's seen-set [(seen_vocab + 31) / 32], or null
    int seen_vocab = 0;           // the sampler's audio_vocab: ids outside [0, seen_vocab) have no bit
    const float* talker_emb = nullptr;
    int talker_vocab = 0;
    const float* const* cp_tables = nullptr;   // device array [n_groups]
    int cp_vocab = 0, n_groups = 15;
    const float* pad_embed = nullptr;
    float* h = nullptr;           // null: the rows are not built (a prefix-cache hit holds what a prefill makes of them)
    float* ssq = nullptr;
    half_t* xh = nullptr;
    const float* gamma = nullptr; // input norm weight of the layer that consumes xh
    int row0 = 0, max_rows = 0, H = 0;
};
int launch_prompt_rows(hipStream_t s, const PromptRowsArgs& a);

// diagnostic timeline build: node numbering of the launches that follow (no-op otherwise)
int tl_next_node();

// ---- dispatch knobs (tests and probes) ----
int set_linear_tuning(int K, int mt16, int kbw);   // k-blocks per wave for (K, row tile); -1: no such entry
int set_linear_split_rows(int on);
int set_linear_narrow8(int on);
int set_linear_wide_tiles(int on);
int set_attn_short(int on);
int set_gemm_min_rows(int n);
int set_gemm_glds(int on);
int reset_linear_knobs();
const char* last_linear_variant();

}  // namespace q3
