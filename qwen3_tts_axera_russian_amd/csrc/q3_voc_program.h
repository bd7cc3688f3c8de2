// q3_voc_program.h -- the vocoder's program as q3_voc.hip holds it, for q3_voc_stream.hip: the op table, the handle, the chunk
// decode (voc_run) and the op -> launch layer both decode walks share.  Internal; the C ABI is include/qwen3tts_voc.h.
#pragma once
#include "q3_common.h"
#include "q3_voc_ops.h"

#include <vector>

namespace q3 {

enum { VOP_RVQ = 1, VOP_CONV = 2, VOP_CONVT = 3, VOP_DWCONV = 4, VOP_NORM = 5, VOP_ATTN = 6, VOP_GLU = 7, VOP_EMBMEAN = 8 };
enum { VF_SNAKE = 1, VF_RES_ADD = 2, VF_RES_SAVE = 4, VF_CLAMP = 8, VF_GELU = 16 };

struct VocOp {
    int op = 0, cin = 0, cout = 0, k = 0, p0 = 0, flags = 0, nq = 0, cb = 0;
    float *w = nullptr, *bias = nullptr, *alpha = nullptr, *inv_beta = nullptr;  // device
    int kind = 0, heads = 0, head_dim = 0, window = 0;   // NORM kind; ATTN geometry
    float eps = 0.f, theta = 10000.f;
    _Float16 *w_hi = nullptr, *w_lo = nullptr;  // split-precision weights (null: exact path only)
    int Mp128 = 0;
    float *p_sem = nullptr, *p_ac = nullptr;
    float* w1p = nullptr;   // 1x1 conv closing a residual unit: A operands in resunit_kernel's K order
    int lt = 0, rt = 0;     // transposed conv: samples trimmed from the (L - 1) * stride + k outputs, left / right
};

// row pitch of an activation: L rounded up to 32 floats = one 128-byte line, so that rows (and the 32-column runs a wave
// stores) start on a line whatever L is -- with a 16-byte pitch the fused units' stores straddled two lines and WRITE_SIZE
// counted 4.5-4.6 B per element instead of 4.00 (profiles/r03_pmc_vocoder.md); the kernels need 4 | pitch only
static inline long pitch4(long L) { return (L + 31) & ~31L; }
// kept outputs of a transposed conv over L input columns
static inline long convt_out(const VocOp& op, long L) { return (L - 1) * op.p0 + op.k - op.lt - op.rt; }
// columns of its polyphase GEMM that reach a kept output (virtual row p of column l lands at l * s + p - lt)
static inline long convt_cols(const VocOp& op, long L) {
    const long lc = (convt_out(op, L) + op.lt + op.p0 - 1) / op.p0;
    return lc < L ? L : lc;
}

struct Voc {
    int device = 0;           // the HIP device the handle was loaded on (q3_set_device before voc_load); entry points bind their thread to it
    VocSettings cfg;          // the settings of the call in flight (voc_enter): all that planning, walks and launchers read
    int chunk = 64, max_batch = 1, upsample = 1;
    long chunk_samples = 0;   // what one decode of `chunk` frames yields (<= chunk * upsample: the transposed convs trim)
    std::vector<VocOp> ops;
    std::vector<void*> allocs;
    hipStream_t s = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int64_t* d_codes = nullptr;
    int* d_ovf = nullptr;          // split path: an activation left the fp16 range (the call is redone exactly)
    bool warned_ovf = false;
    float *buf[3] = {nullptr, nullptr, nullptr};
    _Float16 *plane[4] = {nullptr, nullptr, nullptr, nullptr};   // two {hi, lo} plane sets (split path): a conv's input and output
    size_t buf_elems = 0;
    float last_ms = 0.f;
    double flops_per_chunk = 0.0;
    // chunk walk: assembled waveforms of a request (grown on demand) and the per-batch placement table
    float* d_wave = nullptr;
    int16_t* d_wave16 = nullptr;
    size_t wave_cap = 0, wave16_cap = 0;
    ChunkPlace* d_place = nullptr;   // [max_batch]
    float batch_ms = 0.f;            // GPU time of the last voc_synthesize* / voc_synthesize_batch*
    int batch_chunks = 0;            // chunks it decoded
    // pinned staging of every read-back (voc_read_back): one decode of max_batch chunks; h_ovf: the split path's overflow flag
    char* h_stage = nullptr;
    size_t h_stage_bytes = 0;
    int* h_ovf = nullptr;
    // snapshots of incremental streams' carried state (voc_incr_snapshots): the pool is the handle's, since every VocIncr on it
    // lays a stream's state out the same way (H and hoff come from the op table)
    float* d_snap = nullptr;               // [snap slots][snap_pitch]
    size_t snap_pitch = 0;                 // floats between slots: the state, rounded up to 4 (slots start 16-byte aligned)
    std::vector<long long> snap_frames;    // per slot: frames the saved stream had taken, -1 = empty
    std::vector<char> snap_split;          // per slot: the arithmetic it was saved under
    SnapCopy* d_snap_tab = nullptr;        // voc_incr_restore's entries (grown on demand, with the pool)
    size_t snap_tab_cap = 0;
};

// A handle's buffers, stream and events live on the device it was loaded on.  The HIP current device is a per-THREAD setting that
// starts at 0: a worker thread of a process that drives GPU k (one rank of a multi-GPU job, all GPUs visible) would otherwise launch
// the decode's kernels with the wrong device current.  Every entry point that touches the GPU binds its thread first, and takes
// the call's one snapshot of the process-wide settings (q3_voc_settings.h): nothing below an entry point loads the store.
static inline void voc_enter(Voc* v) {
    if (!v) return;
    int d = -1;
    if (hipGetDevice(&d) != hipSuccess || d != v->device) hipSetDevice(v->device);
    v->cfg = voc_settings.load();
}

// device -> the caller's (pageable) memory through the handle's pinned staging, complete on return
int voc_read_back(Voc* v, void* out, const void* dev, size_t bytes);
// T: frames per chunk of THIS decode (0 = the model's chunk length); codes in v->d_codes ([B][T][16]); see q3_voc.hip
int voc_run(Voc* v, int B, float** out_dev, int n_ops = -1, int* outC = nullptr, long* outL = nullptr, float* op_ms = nullptr,
            bool force_exact = false, int T = 0);

// op -> launch.  Each takes an op, explicit buffers and the columns of one entry ([B][C][pitch4(cols)]) and issues the launch
// (0 ok / <0 error); none knows which buffer is current, what a stream carries, or whether a walk only sizes its buffers.
int voc_op_embed(const Voc* v, const VocOp& op, const int64_t* codes, float* out, int T, int B);               // VOP_RVQ / VOP_EMBMEAN
int voc_op_pointwise(const Voc* v, const VocOp& op, const float* in, float* out, long cols, int B);            // VOP_DWCONV / NORM / GLU
// VOP_CONV / VOP_CONVT over `cols` input columns: everything but x, y, res.  Lf: the op's input length in a full-chunk decode
// (ConvArgs::Lrule).  A transposed conv gets the whole-chunk geometry (lt = op.lt, Lout = convt_out, Lc = convt_cols).
ConvArgs voc_conv_args(const VocOp& op, long cols, long Lf);
// The split-precision path of a conv op (launch_conv_split), for voc_run and the incremental walk alike:
bool voc_split_capable(const VocOp& op);                               // built for it: 16 | Cin and every weight inside the fp16 range
// does the split conv `op` hand its result to `next` (the op after it in this walk; null at its end) as input planes from its
// own epilogue?  (The caller adds what only it knows: the incremental walk needs f32 where `next` prepends a history.)
bool voc_split_emits_planes(const VocOp& op, const VocOp* next);
SplitArgs voc_split_args(const VocOp& op, long cols);                  // everything but the planes, y, res and ovf (whole-chunk geometry)
void voc_split_out_planes(SplitArgs& sa, const VocOp& next, _Float16* oh, _Float16* ol);   // the epilogue's planes, next's Snake applied
int voc_split_taps(const VocOp& op);                                   // launch_conv_split's K
// the residual unit op (7 taps) + op1 (the 1x1 conv that closes it) in one launch
ResUnitArgs voc_resunit_args(const VocOp& op, const VocOp& op1, const float* in, float* out, long cols);
// does op i open a residual unit that runs fused (launch_resunit, then skip op i + 1) in a walk of the first n_ops ops?
bool voc_fused_unit(const Voc* v, size_t i, size_t n_ops);

}  // namespace q3
