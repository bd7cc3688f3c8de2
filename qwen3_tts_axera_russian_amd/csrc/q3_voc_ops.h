// q3_voc_ops.h -- the launchers of q3_voc_kernels.hip (a kernel and its launcher share that file) and their argument blocks.
// Used by the vocoder's program (q3_voc.hip), its streaming entry points (q3_voc_stream.hip) and the speech-tokenizer encoder
// (q3_enc.hip, the f32 launchers; its own kernels live in q3_enc.hip).  Every launcher: 0 ok / <0 error (logged).  The conv
// launchers take the caller's settings snapshot (q3_voc_settings.h): the grid cap and the tile rules' knobs.
#pragma once
#include <hip/hip_runtime.h>

#include "q3_voc_settings.h"

namespace q3 {

struct ConvArgs {
    const float* x = nullptr;   // [B][Cin][Lin]
    float* y = nullptr;         // [B][Cout][Lin*stride]
    const float* wk = nullptr;  // [Cin/8][K][8][Mp]: rows contiguous (Mp = M rounded up to 4), M = Cout*stride virtual rows
    int Mp = 0;
    const float* bias = nullptr;
    const float* alpha = nullptr;     // [Cin] Snake: x + inv_beta * sin^2(alpha x), applied to the input
    const float* inv_beta = nullptr;
    const float* res = nullptr;       // [B][Cout][L] added in the epilogue
    int gelu = 0;                     // exact GELU applied to the input (ConvNeXt's second pointwise conv)
    int Cin = 0, M = 0, K = 0, dil = 1, Lin = 0, stride = 1, Cout = 0, clamp = 0;
    // Activations are [B][C][ld]: rows of L valid columns at a pitch ld = L rounded up to 32 floats (pitch4()), so that
    // every row starts on a 128-byte line whatever L is (the transposed convs of the decoder family trim k - s samples at both ends:
    // 64 frames -> 256 -> 2040 -> 10195 -> 40776 -> 122325 columns).  Pad columns hold junk that only ever feeds pad
    // columns: every op is causal per column (a GEMM column depends on its own B column only).
    int ldx = 0, ldy = 0;
    // transposed conv: virtual row m = co * stride + p of input column l lands at output column l * stride + p - lt
    // (lt samples trimmed on the left), kept when 0 <= that < Lout; Lc = columns of the polyphase GEMM that reach a
    // kept output (= Lin for the trims in use; inputs at l >= Lin read as zero)
    int lt = 0, Lout = 0, Lc = 0;
    // Lc of this op when the decode runs the full chunk length: the launcher's variant rule looks at it, so that a decode of
    // fewer frames (voc_run's T) sums every column in the same order as the full-length one (0: use Lc)
    int Lrule = 0;
    int n_tiles = 0, tiles_l = 0, tiles_m = 0;  // set by the launcher
    // one-tap, stride-1 convs (pointwise projections): the columns of all B chunks form ONE axis of B*Lin columns
    // (a column needs no neighbour), so 128-column tiles stay full when a chunk is only 64 columns long
    int flat_B = 0;                              // > 0: flattened, B chunks
    // ELU on the input while it is staged (the encoder's SEANet convs; ELU(0) = 0, so the causal zero padding commutes).
    // Built for 1- and 3-tap convs over a multiple of 16 input channels, at 16 channels per stage only: the stage width
    // fixes the order in which a 3-tap conv sums taps and channels, so a column's bits never depend on the batch
    int elu = 0;
};

// causal Conv1d / polyphase ConvTranspose1d on the exact-fp32 MFMA (conv_kernel and its one-row form)
int voc_launch_conv(hipStream_t s, const ConvArgs& a, int B, const VocSettings& cfg);
// RMSNorm (kind 0) / LayerNorm (kind 1) over the C channels of every column of x [B][C][ld] (L columns)
int voc_launch_norm(hipStream_t s, const float* x, const float* w, const float* bias, float* y, int C, int L, int ld,
                    int kind, float eps, int B);
// causal sliding-window attention with rotate-half RoPE, x = [q | k | v] head-major [B][3*H*D][ld] -> y [B][H*D][ld].
// One wave per (query column, head) walks its keys in order: a column's bits do not depend on L or B.
int voc_launch_attn(hipStream_t s, const float* x, float* y, int H, int D, int L, int ld, int window, float theta, int B);
// The same attention with one workgroup per (head, batch entry) holding the head's q, k, v in LDS (voc_attn_tile_kernel,
// the vocoder's variant for short chunks): head_dim even and <= 64, 3 * L * (D + 1) floats <= 64 KiB; -1 otherwise.
// Exposed for the kernel-level test hook.
int voc_launch_attn_tile(hipStream_t s, const float* x, float* y, int H, int D, int L, int ld, int window, float theta, int B);

// fused residual unit y = x + conv1x1(Snake(conv7(Snake(x)))) (resunit_kernel), built for the channel counts of resunit_channels
struct ResUnitArgs {
    const float* x = nullptr;     // [B][C][Lin]
    float* y = nullptr;           // [B][C][Lin]
    const float* w7 = nullptr;    // [C/8][7][8][C]   (conv_kernel's stage-major layout)
    const float* w1p = nullptr;   // [C/32][C/2][64]  (A operands of the 1x1 conv in the order above)
    const float *b7 = nullptr, *b1 = nullptr;                    // biases (may be null)
    const float *al7 = nullptr, *ib7 = nullptr;                  // Snake of the unit's input
    const float *al1 = nullptr, *ib1 = nullptr;                  // Snake between the convs
    int Lin = 0, ld = 0, dil = 1, tiles_l = 0, n_tiles = 0;   // ld: row pitch of x and y (ConvArgs)
};
bool resunit_channels(int c);
int launch_resunit(hipStream_t s, const ResUnitArgs& a, int C, int B, const VocSettings& cfg);

// split-precision conv on the fp16 MFMA (conv_split_kernel) over {hi, lo} fp16 planes; K taps
struct SplitArgs {
    const _Float16* xh = nullptr;        // [B][Cin/8][Lin][8]
    const _Float16* xl = nullptr;
    float* y = nullptr;                  // [B][Cout][Lin*stride] f32
    const _Float16* w_hi = nullptr;      // [Cin/16][K][Mp][16]  (Mp = rows padded to 128)
    const _Float16* w_lo = nullptr;
    const float* bias = nullptr;
    const float* res = nullptr;
    // optional second output (stride 1 only): the result already in the NEXT conv's input form -- its Snake
    // applied, split into hi/lo planes [B][Cout/8][Lin][8] -- so no separate pass re-reads it
    _Float16* oh = nullptr;
    _Float16* ol = nullptr;
    const float* oalpha = nullptr;
    const float* oinv_beta = nullptr;
    int* ovf = nullptr;                  // set to 1 when an output plane value leaves the fp16 range
    int ovf_stride = 0;                  // entry b raises ovf[b * ovf_stride]: 0 = one flag for the call, 1 = a flag per entry
    int Cin = 0, M = 0, Mp = 0, dil = 1, Lin = 0, stride = 1, Cout = 0, clamp = 0, B = 0;
    int ldy = 0, lt = 0, Lout = 0, Lc = 0;   // f32 output pitch, left trim / kept outputs / GEMM columns (ConvArgs)
    int n_tiles = 0, tiles_l = 0, tiles_m = 0;
    int my_fast = 0;   // tile order, see conv_split_kernel
};
int launch_conv_split(hipStream_t s, const SplitArgs& a, int K, int B, const VocSettings& cfg);
// x f32 [B][C][ld] -> Snake / GELU -> the planes a split conv reads; ovf[b * ovf_stride] = 1 when a value of entry b leaves the
// fp16 range (SplitArgs::ovf_stride)
int voc_launch_snake_split(hipStream_t s, const float* x, const float* alpha, const float* inv_beta, _Float16* xh, _Float16* xl, int C,
                           int L, int ld, int gelu, int* ovf, int B, int ovf_stride = 0);

// the small f32 ops over x [B][C][ld] (L columns), and the two code-id front ends (codes [B][T][16])
int voc_launch_dwconv(hipStream_t s, const float* x, const float* w, const float* bias, float* y, int C, int L, int ld, int K, int B);
int voc_launch_glu(hipStream_t s, const float* x, float* y, int C, int L, int ld, int act, int B);
int voc_launch_rvq(hipStream_t s, const int64_t* codes, const float* cb, const float* p_sem, const float* p_ac, float* y, int T, int ld,
                   int NQ, int CB, int DIM, int OUT, int B);
int voc_launch_embmean(hipStream_t s, const int64_t* codes, const float* tab, float* y, int T, int ld, int NQ, int NQS, int CB, int DIM, int B);

// chunk walk: B decoded chunks (rows of dec) land in the assembled waveform, copy then cross-fade (two launches)
struct ChunkPlace {
    int row;            // row of the decode batch's output
    int len;            // samples of the chunk after the reference's slice (min(frames * 1920, chunk_samples))
    int head;           // 0: plain append; OV: the first OV samples are cross-faded into what is already there
    long long dst;      // sample index in the batch output buffer where the chunk's first sample lands
};
int voc_launch_place(hipStream_t s, const float* dec, int pitch, const ChunkPlace* pl, float* out, int OV, int B);
int voc_launch_to_int16(hipStream_t s, const float* x, int16_t* y, long long n);

// streaming chunk walk: n windows of the work buffer; emit writes int16 (want16) or f32 samples to out
struct StreamWin {
    long long win;      // first sample of the stream's window in the work buffer
    long long out;      // first sample of its part of the packed output
    long long n_out;    // samples handed out
    int stream;         // tail slot
    int tail_in;        // samples of the kept tail loaded to the window's front (0 or OV)
    int tail_out;       // samples kept after the handed-out ones (0 when the stream finishes, else OV)
};
int voc_launch_stream_load(hipStream_t s, const float* tail, int OV, const StreamWin* w, float* work, int n);
int voc_launch_stream_emit(hipStream_t s, const float* work, const StreamWin* w, float* tail, int OV, void* out, bool want16, int n);

// incremental decode: [history | new] assembly, attention over the carried window, packed output (int16 or f32).  The history
// of entry b is read from hist{parity[b]} and written to the other buffer; parity == nullptr: hist0, in place.
int voc_launch_incr_prepend(hipStream_t s, const float* src, int src_C, int c0, int src_ld, int skip, float* dst, int C, int dst_ld,
                            float* hist0, float* hist1, const int* parity, int H, int n, long long state_floats, const int* streams, int B);
// [history | new] of all C channels as the consuming split conv's input planes (its Snake / GELU applied), and as f32 where dst
// is given; ovf[b] = 1 when a plane value of entry b leaves the fp16 range.  Two history buffers only (parity given).
int voc_launch_incr_prepend_split(hipStream_t s, const float* src, int src_ld, int skip, _Float16* xh, _Float16* xl, float* dst, int dst_ld,
                                  int C, const float* alpha, const float* inv_beta, int gelu, float* hist0, float* hist1, const int* parity,
                                  int H, int n, long long state_floats, const int* streams, int* ovf, int B);
int voc_launch_incr_attn(hipStream_t s, const float* x, int x_ld, int skip, const float* kv, int kv_ld, int Hk, float* y, int H, int D,
                         int window, float theta, const int* pos0, int n, int B);
int voc_launch_incr_emit(hipStream_t s, const float* y, int ld, int skip, int n, const long long* out_off, void* out, bool want16, int B);

// snapshot restore: n entries of a device table, each `floats` floats from a slot into a stream's history (dst1: the second
// history buffer of a double-buffered object, or null), in one launch
struct SnapCopy {
    const float* src;
    float* dst0;
    float* dst1;
};
int voc_launch_incr_restore(hipStream_t s, const SnapCopy* tab, long long floats, int n);

}  // namespace q3
