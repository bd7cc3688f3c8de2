// q3_model.h -- device-resident model, KV cache, workspaces and the layer-stack runner.
#pragma once
#include "q3_kernels.h"

namespace q3 {

struct DevLinear {
    half_t* wp = nullptr;  // fragment-packed fp16
    int N = 0, K = 0;
};

struct DevLayer {
    DevLinear qkv, o, gu, down;
    float *in_ln = nullptr, *post_ln = nullptr, *q_norm = nullptr, *k_norm = nullptr;
};

struct DevStack {
    std::vector<DevLayer> L;
    float* final_norm = nullptr;
    // norm weight of whatever consumes the stack's output THROUGH A GEMM (code predictor: final_norm, the group
    // heads read the last layer's xh); null when the output is only normed element-wise (talker)
    const float* tail_gamma = nullptr;
    int ffn = 0;
    int nt = 0;  // non-temporal weight stream
    size_t weight_bytes = 0;
};

struct Model {
    ModelCfg cfg;
    int device = 0;
    bool has_talker = false, has_cp = false;
    DevStack talker, cp;
    float* talker_emb = nullptr;  // f32 [talker_vocab][hidden]
    DevLinear talker_head;
    std::vector<float*> cp_emb;   // f32 [cp_vocab][hidden] each
    std::vector<DevLinear> cp_head;
    const float** d_cp_emb_ptrs = nullptr;  // device array of the cp_emb pointers
    // Layer 0's q|k|v of the code predictor for every row of cp_emb[0 .. cp_groups-2]: f32 [cp_groups-1][cp_vocab][qkv_ld],
    // the exact bits of run_stack's PRO_NORM / EPI_STORE launch on that embedding row, built at load by that launch
    // itself (positions 2.. of a frame embed a code-predictor token, so this launch is a function of (group, token)).
    // Null with Q3_CP_QKV_TABLE=0.  cp_qkv_kbw: the K split (linear_decode_kbw) its rows were summed with -- a pass whose
    // row count would split K differently keeps the live launch.
    float* cp_qkv_tab = nullptr;
    int cp_qkv_kbw = 0;
    const float* cp_qkv_rows(int group) const {   // table of the tokens of cp_emb[group]
        return cp_qkv_tab + (size_t)group * cfg.cp_vocab * ((cfg.n_heads + 2 * cfg.n_kv) * cfg.head_dim);
    }
    // whether a pass of `rows` rows may take layer 0's q|k|v from the table
    bool cp_qkv_serves(int rows) const {
        return cp_qkv_tab && linear_decode_kbw(cfg.hidden, (cfg.n_heads + 2 * cfg.n_kv) * cfg.head_dim, rows) == cp_qkv_kbw;
    }
    float *rope_cos = nullptr, *rope_sin = nullptr;  // [max_pos][head_dim/2]
    int max_pos = 0;
    std::vector<void*> allocs;
    size_t device_bytes = 0;
};

// `path`: a Q3TTSW1 container, or the reference's own files (Pack::open_auto); `aux_dir`: its --embeddings_dir.  `s`: the
// stream the uploads and the repacking kernels run on (synchronised before the return); null = a stream of the loader's
// own, destroyed when loading ends.  An owner that passes its stream keeps loading off every other hardware queue.
Model* model_load(const char* path, bool want_talker, bool want_cp, const char* aux_dir = nullptr, hipStream_t s = nullptr);
void model_free(Model* m);

// ggml blocks of `type` (Q4_0 .. Q6_K of DType), already on the device -> n_rows x K row-major values, as fp16 (round to
// nearest even, saturating at +-65504) when out_f16 is set or as the fp32 value itself when out_f32 is: exactly one of the
// two.  K is a multiple of the block; both outputs are 16-byte aligned.  *flag (device) is set to 1 when a block's scale is
// Inf or NaN, and is otherwise left alone: the caller zeroes it.  Asynchronous on s.  (csrc/q3_dequant.hip)
int launch_dequant(hipStream_t s, uint32_t type, const uint8_t* blocks, size_t n_rows, size_t K, half_t* out_f16, float* out_f32,
                   int* flag);

struct KVCache {
    half_t *k = nullptr, *v = nullptr;
    int n_layers = 0, n_slots = 0, n_kv = 0, n_ctx = 0, head_dim = 128;
    size_t layer_stride() const { return (size_t)n_slots * n_kv * n_ctx * head_dim; }
    size_t bytes() const { return layer_stride() * n_layers * sizeof(half_t) * 2; }
};
int kv_alloc(KVCache& kv, int n_layers, int n_slots, int n_kv, int n_ctx, hipStream_t s = nullptr);   // zeroed on s, synchronised
void kv_free(KVCache& kv);
int kv_zero(hipStream_t s, KVCache& kv);   // every slot's keys and values to 0 (asynchronous on s)

// Activations of one stack pass over up to max_rows rows (fragment order: frag_idx, q3_frag.h).
struct Work {
    int max_rows = 0, hidden = 0;   // max_rows is padded to a multiple of 128 (largest row tile)
    float* rows_in = nullptr;       // row-major staging of uploaded embedding rows
    float *h = nullptr, *ssq = nullptr, *qkv = nullptr;   // h: fragment order
    half_t* xh = nullptr;          // fp16((h*gamma_consumer)/16), fragment order: the next normed GEMM's input
    half_t *attn = nullptr, *act = nullptr;
    float* hidden_f32 = nullptr;   // post-final-norm
    half_t* hidden_f16 = nullptr;
    float* logits = nullptr;       // [max_rows][max vocab]
    // (slot, position) of the rows of the code predictor's two-position first pass (cp_frame): rows [0, R16) are
    // position 1, rows [R16, 2*R16) position 0 of slots 0..R16-1; filled for map_R16
    int *map_slot = nullptr, *map_pos = nullptr;
    int map_R16 = 0;
};
int work_alloc(Work& w, const ModelCfg& c, int max_rows, int ffn, int max_vocab, hipStream_t s = nullptr);   // zeroed on s, synchronised
void work_free(Work& w);
// every activation buffer of w to 0 (asynchronous on s; ffn / max_vocab as for work_alloc): no row reads uninitialised memory
int work_zero(hipStream_t s, Work& w, const ModelCfg& c, int ffn, int max_vocab);

struct RowMap {            // which (slot, position) each row feeds
    const int* slot = nullptr;  // device [R] or null -> slot_base + r*slot_stride
    const int* pos = nullptr;   // device [R] or null -> pos_base + r*pos_stride
    int slot_base = 0, slot_stride = 0, pos_base = 0, pos_stride = 0;
    bool same_slot_rows = false;  // rows depend on each other through the cache (prefill): split prep/attend
    int valid_mod = 0, valid_n = 0;  // rows r with (r % valid_mod) >= valid_n are padding (AttnArgs)
    // same_slot_rows: the rows as runs of <= 16 consecutive positions of one slot (device int[4] per tile: first row,
    // rows, slot, first position); without a table a pass with slot_stride 0 / pos_stride 1 is tiled implicitly
    const int* tiles = nullptr;
    int n_tiles = 0;
    // layer 0's q|k|v rows already sit in w.qkv (cp_frame: copied from Model::cp_qkv_tab by the producer of h): that
    // launch is left out
    bool skip_qkv0 = false;
    // rows of the whole step when this pass covers one row group of it (parallel chains): the attention launch is shaped
    // for that many rows, so a row sums its cached positions in the same order whichever group it runs in.  0 = R.
    int rows_total = 0;
};

// Run every layer of `st` over R rows whose residual stream (+ssq partials) sits in w.h / w.ssq.
int run_stack(hipStream_t s, const Model& m, const DevStack& st, Work& w, KVCache& kv, int R,
              const RowMap& rm, int attn_threads, int row0 = 0);

struct GraphExec {
    hipGraph_t g = nullptr;
    hipGraphExec_t e = nullptr;
    void reset();
    // Capture what body() (-> 0 ok) launches on s and instantiate it, in place of whatever was held; `who` names the caller
    // in the log.  The caller has run the body eagerly once before (the kernels' attributes are set outside a capture).
    template <class F>
    int capture(hipStream_t s, hipStreamCaptureMode mode, const char* who, F&& body) {
        reset();
        Q3_HIP(hipStreamBeginCapture(s, mode), -1);
        return end_capture(s, body(), who);
    }

private:
    int end_capture(hipStream_t s, int body_rc, const char* who);
};

}  // namespace q3
