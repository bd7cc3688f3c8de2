// q3_voc_ops.h -- the vocoder's f32 op launchers that the speech-tokenizer encoder (q3_enc.hip) shares.
// Defined in q3_voc.hip; the encoder's own kernels live in q3_enc.hip.
#pragma once
#include <hip/hip_runtime.h>

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

// causal Conv1d (stride 1) on the exact-fp32 MFMA (conv_kernel): 0 ok / <0 error (logged)
int voc_launch_conv(hipStream_t s, const ConvArgs& a, int B);
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

}  // namespace q3
