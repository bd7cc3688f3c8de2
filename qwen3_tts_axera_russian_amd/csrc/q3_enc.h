// q3_enc.h -- what the encoder's two translation units share: the loaded op table (q3_enc.hip builds it, q3_enc_stream.hip
// walks it a push at a time), the op -> launch layer under both walks (enc_conv_args, and the launchers of the kernels that
// q3_enc.hip defines: the first conv and the quantiser), and the host arithmetic of the streaming encode (no device call: the
// test library hands it to the CPU tests as it stands).
#pragma once
#include "q3_common.h"
#include "q3_voc_ops.h"

#include <vector>

namespace q3 {

enum { EOP_CONV_IN = 1, EOP_CONV = 2, EOP_CONV_S = 3, EOP_NORM = 4, EOP_ATTN = 5, EOP_RVQ = 6 };
enum { EF_ELU = 1, EF_RES_SAVE = 2, EF_RES_ADD = 4, EF_TO_RES = 8, EF_GELU = 16, EF_REPLICATE = 32 };

static inline long enc_pitch(long L) { return (L + 31) & ~31L; }

constexpr int ENC_IN_MAXK = 16;

struct EncOp {
    int op = 0, cin = 0, cout = 0, k = 0, p0 = 0, flags = 0;   // p0: dilation (CONV) / stride (CONV_S)
    int c_act = 0;                                            // channels of the activation after the op (a TO_RES shortcut keeps its input's)
    float *w = nullptr, *bias = nullptr;                      // conv weights in conv_kernel's packed layout (CONV_IN: [cout][k])
    int heads = 0, head_dim = 0, window = 0;
    float eps = 0.f, theta = 10000.f;
    int nq = 0, cb = 0, dim = 0, n_sem = 0;                    // RVQ
    float *cbk = nullptr, *cbt = nullptr, *n2 = nullptr;
};

struct Enc {
    int device = 0;
    VocSettings cfg;                // the call's snapshot of the process-wide settings (enc_enter): voc_launch_conv's grid cap and fill
    int max_batch = 1, max_samples = 0, sample_rate = 24000, hop = 1, nq = 0;
    std::vector<EncOp> ops;
    DeviceAllocs mem;
    hipStream_t s = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    float* pcm = nullptr;           // [max_batch][pitch(max_samples)]
    float* buf[4] = {nullptr, nullptr, nullptr, nullptr};   // ping-pong pair, residual, unfolded input
    size_t buf_elems = 0;
    int* d_lens = nullptr;          // [n_ops][max_batch] per-clip input lengths of every op
    int64_t* d_codes = nullptr;     // [max_batch][max frames][nq]
    size_t codes_cap = 0;
    float last_ms = 0.f;
    // the PCM front-end (q3_enc_pcm.hip): the payload as the client sent it, the clips' geometry, the tap tables built so far
    struct PcmTable {
        int up = 0, down = 0;
        double* taps = nullptr;     // [per_phase][up], q3_enc_pcm_host.h
        uint64_t used = 0;          // the call that read it last (the least recent one goes when a fifth comes)
    };
    void* pcm_raw = nullptr;
    size_t pcm_raw_bytes = 0;
    long long* pcm_meta = nullptr;  // [max_batch][3]: first frame, input frames, output samples
    std::vector<long long> pcm_meta_host;
    std::vector<PcmTable> pcm_tables;
    uint64_t pcm_calls = 0;
};

// every entry point that touches the GPU: binds the thread to the handle's device and takes the call's one settings snapshot
// (q3_voc_settings.h; the walks pass it to voc_launch_conv)
static inline void enc_enter(Enc* e) {
    if (!e) return;
    int d = -1;
    if (hipGetDevice(&d) != hipSuccess || d != e->device) hipSetDevice(e->device);
    e->cfg = voc_settings.load();
}

// the columns an op hands on from L: a strided conv pads a clip's end to whole strides, ceil(L / s)
static inline long enc_cols_out(const EncOp& op, long L) { return op.op == EOP_CONV_S ? (L + op.p0 - 1) / op.p0 : L; }
static inline long enc_cols_after(const std::vector<EncOp>& ops, size_t n_ops, long L) {
    for (size_t i = 0; i < n_ops; i++) L = enc_cols_out(ops[i], L);
    return L;
}

// A conv op over `cols` columns as voc_launch_conv takes it, all but x, y and res.  unfolded: a strided op as the 1-tap conv
// over the [cin * k] rows of its unfold kernel.
static inline ConvArgs enc_conv_args(const EncOp& op, long cols, bool unfolded) {
    ConvArgs a;
    a.Cin = unfolded ? op.cin * op.k : op.cin;
    a.K = unfolded ? 1 : op.k;
    a.dil = unfolded ? 1 : op.p0;
    a.elu = (!unfolded && (op.flags & EF_ELU)) ? 1 : 0;   // (the unfold kernel has applied a strided op's ELU)
    a.gelu = (!unfolded && (op.flags & EF_GELU)) ? 1 : 0;
    a.wk = op.w;
    a.bias = op.bias;
    a.Cout = a.M = op.cout;
    a.stride = 1;
    a.Lin = a.Lout = a.Lc = (int)cols;
    // Never the short-activation variants: the launcher's variant rule reads Lrule, so pinned it depends on nothing in the
    // call -- not the columns, the batch or the split of a stream.  "Clip b gives the same bits alone, in a batch and in any
    // split" rests on this line.
    a.Lrule = 1 << 20;
    a.ldx = a.ldy = (int)enc_pitch(cols);
    return a;
}

// the first conv: x [B][ldx], n columns of the one input channel -> y [B][cout][ldy].  hist == nullptr: a whole clip (zeros left
// of column 0); else entry b continues stream streams[b], whose last k - 1 samples are at hist + streams[b] * state_floats
int enc_launch_conv_in(hipStream_t s, const float* x, int ldx, const EncOp& op, float* y, int ldy, int n, int B, float* hist,
                       long long state_floats, const int* streams);
// a strided conv's input of whole clips: x [B][Cin][ldx], clip b's own length lens[b] (device) -> y [B][Cin * k][pitch(Lout)],
// columns below Lout (enc_unfold_kernel states the padding)
int enc_launch_unfold(hipStream_t st, const float* x, int ldx, int Cin, const int* lens, float* y, int Lout, int k, int s, int replicate,
                      int elu, int B);
// the same of one push (q3_enc_stream.hip, enc_stream_unfold_kernel): n_in new columns of x [B][Cin][ldx] from column skip behind
// the carry of stream streams[b], `before[b]` columns taken so far -> y [B][Cin * k][pitch(n_out)]; the carry row
// hist + streams[b] * state_floats + ci * (k - 1) moves on unless the push finishes
int enc_stream_launch_unfold(hipStream_t st, const float* x, int ldx, int skip, int Cin, int n_in, float* y, int n_out, int k, int s,
                             int replicate, int elu, int finish, float* hist, long long state_floats, const int* streams, const int* before,
                             int B);
// columns [skip, skip + n) of y [B][C][ld] -> rows off[b] + j of out [frames][C]
int enc_stream_launch_emit(hipStream_t st, const float* y, int C, int ld, int skip, int n, const int* off, float* out, int B);
// the split residual VQ over n_frames frames, frame g = b * T + t read from z [B][2 * dim][ld] -> codes [n_frames][nq]
int enc_launch_rvq(hipStream_t s, const float* z, int ld, int T, int n_frames, const EncOp& op, int64_t* codes);
// frames per workgroup of that launch: enc_rvq_kernel<16> from 2048 frames, enc_rvq_kernel<4> below.  A frame's ids do not
// depend on the width (per frame, one fma chain over d in order).
static inline int enc_rvq_tile(int n_frames) { return n_frames >= 2048 ? 16 : 4; }
// the quantiser geometry enc_load admits (its input is the 2 * dim rows semantic | acoustic)
static inline bool enc_rvq_geometry(int nq, int cb, int dim, int n_sem) {
    return nq >= 1 && nq <= 32 && cb >= 1 && dim >= 4 && dim % 4 == 0 && dim <= 1024 && n_sem >= 1 && n_sem <= nq;
}
// the quantiser's device tables from the host codebook [nq][cb][dim] (finite; op.nq, op.cb and op.dim set): op.cbk the codebook,
// op.cbt its transpose [nq][dim][cb], op.n2 [nq][cb] = (float) of the double sum of squares.  -> false: an allocation or a copy failed
bool enc_rvq_tables(DeviceAllocs& mem, const float* codebook, EncOp& op);

// ---- what enc_encode and enc_encode_pcm share (q3_enc.hip) ----
// runs ops [0, n_ops) (n_ops < 0: all) on the B clips already in e->pcm: rows of pitch enc_pitch(longest), each zero past its
// own lens[b] samples.  -> the buffer of the last activation (nullptr after the quantiser), its channels and longest length
int enc_run(Enc* e, int B, const std::vector<int>& lens, int n_ops, float** out, int* outC, long* outL);
// after enc_run's quantiser: the ids to the host, e1 recorded, the stream drained, last_ms = e0 -> e1, codes_out / n_frames
// filled as enc_encode documents them (T: enc_run's outL)
int enc_collect_codes(Enc* e, int B, const std::vector<int>& lens, long T, int64_t* codes_out, int max_frames, int32_t* n_frames);
// enc_destroy's part for the front-end's own allocations (q3_enc_pcm.hip)
void enc_pcm_release(Enc* e);

// ---- streaming encode: the column counts of every level from a stream's running total ----
// Level l is the input of the l-th strided op (level 0: samples); cols[n_levels] are frames.  A strided op of stride s turns
// the T columns it has been given into floor(T / s) outputs while the stream runs -- output u reads inputs below (u + 1) * s --
// and into ceil(T / s) once the stream has finished (the leftover padded as a clip's end is).  Nested floors (and nested
// ceilings) compose, so every level follows from the total alone.
static inline void enc_stream_cols(const int* strides, int n_levels, long long total, bool finished, long long* cols) {
    long long L = total;
    for (int l = 0; l < n_levels; l++) {
        cols[l] = L;
        L = finished ? (L + strides[l] - 1) / strides[l] : L / strides[l];
    }
    cols[n_levels] = L;
}

// What one push does to a stream that had `before` samples: n_in[l] new columns at level l (n_in[n_levels]: frames handed
// out), before_cols[l] the columns level l had taken, and carry[l] the columns strided op l holds when the push starts: its
// k - s left-context columns plus the before_cols[l] % s not yet consumed by a whole stride.
static inline void enc_stream_plan(const int* ks, const int* strides, int n_levels, long long before, long long n_new, bool finish,
                                   long long* n_in, long long* before_cols, long long* carry) {
    std::vector<long long> a(n_levels + 1);
    enc_stream_cols(strides, n_levels, before, false, before_cols);
    enc_stream_cols(strides, n_levels, before + n_new, finish, a.data());
    for (int l = 0; l <= n_levels; l++) n_in[l] = a[l] - before_cols[l];
    for (int l = 0; l < n_levels; l++) carry[l] = (ks[l] - strides[l]) + before_cols[l] % strides[l];
}

// ---- the streaming encode's object (q3_enc_stream.hip; q3_enc_stream_pcm.hip feeds it) ----
struct EncStreamPcm;
enum { ENC_SRC_NONE = 0, ENC_SRC_F32 = 1, ENC_SRC_PCM = 2 };   // what has fed a stream since its reset
struct EncStream {
    Enc* e = nullptr;
    int max_streams = 0, max_push = 0;
    std::vector<long long> total;         // samples a stream has taken since its reset
    std::vector<char> finished;
    std::vector<char> source;             // ENC_SRC_*: enc_stream_push and enc_stream_push_pcm do not mix on one clip
    std::vector<int> lev_k, lev_s;        // the strided ops' taps and strides, in order
    std::vector<int> level_of;            // per op: the level of its input
    std::vector<int> H;                   // per op: carried columns (0: nothing)
    std::vector<size_t> hoff;             // per op: offset of its [channels][H] block inside a stream's state
    size_t state_floats = 0;
    float* d_hist = nullptr;              // [max_streams][state_floats]
    float* buf[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t buf_elems = 0, kv_elems = 0;   // floats of one work buffer / of d_kv (without the slack)
    float* d_kv = nullptr;                // attention: [carried window | new] k and v rows
    float* d_pcm = nullptr;               // [max_batch][pitch(max_push)]
    int* d_meta = nullptr;                // [2 + n_ops][max_batch]: streams, per op the columns its level had taken, frame offsets
    float* d_z = nullptr;                 // [frames_cap][2 * dim]: the quantiser's input of the whole push
    float* d_emb = nullptr;               // [frames_cap][emb_C]: the pre-quantiser embedding (test hook)
    int64_t* d_codes = nullptr;           // [frames_cap][nq]
    size_t frames_cap = 0;
    int emb_op = -1, emb_C = 0;           // the op whose input is the embedding (the projection before the quantiser)
    DeviceAllocs mem;
    float last_ms = 0.f;
    int last_launches = 0;
    EncStreamPcm* pcm = nullptr;          // the PCM front-end's carry rows, from the first enc_stream_push_pcm on (not in `mem`)
};

// A push whose samples do not come from the host: the feed writes entry b's n 24 kHz samples into row b of d_pcm, from
// column 0 on, where the walk's first conv reads them.  Each call returns the kernel launches it made, or < 0.
struct EncStreamFeed {
    virtual ~EncStreamFeed() = default;
    virtual int begin() = 0;   // the push is valid and nothing has been written yet: uploads (a failure refuses the push)
    virtual int fill(const std::vector<int>& members, long long n) = 0;   // one group (entry indices) of n > 0 samples each
    virtual int end() = 0;     // after the last group's walk
};

// enc_stream_push with one more output (the test library's q3t_enc_stream_embeddings): emb_out, when given, receives the
// pre-quantiser embedding columns of the push, [frames][channels] packed like the codes.  feed: n_new are the 24 kHz counts
// of a push the feed supplies (pcm is not read)
int enc_stream_push_impl(EncStream* s, int n, const int32_t* streams, const float* pcm, const int32_t* n_new, const int32_t* finish,
                         int64_t* codes_out, int64_t out_capacity_frames, int64_t* offsets, float* emb_out, int* emb_channels,
                         EncStreamFeed* feed = nullptr);
// enc_stream_push_max_frames for a push from `source`; < 0 refused (logged)
int enc_stream_plan_frames(const EncStream* s, int n, const int32_t* streams, const int32_t* n_new, const int32_t* finish, int source);
// enc_stream_free's part for the front-end's allocations (q3_enc_stream_pcm.hip)
void enc_stream_pcm_release(EncStream* s);

// ---- the PCM front-end's device tables, shared by enc_encode_pcm and enc_stream_push_pcm (q3_enc_pcm.hip) ----
struct EncPcmPlan;
// the device table of the plan: one the handle kept, or built now in place of the least recently used
const double* enc_pcm_table(Enc* e, const EncPcmPlan& p);
// e->pcm_raw holds at least `bytes` (it grows to the largest payload seen); false: no memory, logged under `who`
bool enc_pcm_raw_reserve(Enc* e, size_t bytes, const char* who);

}  // namespace q3
