// q3_frag.h -- the fragment order of GEMM operands, one function for kernels and host code (a plain inline function to a
// host compiler: the host-only drivers of tests/ include it through q3_kernels.h).
#pragma once
#include <cstddef>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define Q3_FRAG_FN __host__ __device__ __forceinline__
#else
#define Q3_FRAG_FN inline
#endif

namespace q3 {

// Activations that feed a GEMM (residual stream h, attention output, SwiGLU output) live in MFMA
// A-fragment order, like the weights: 16-row x 32-k blocks (mt = m/16, kb = k/32), inside a block lane
// (m%16) + 16*((k%32)/8) owns 8 consecutive k.  A wave's fragment load is then 64 lanes x 16 B (fp16) or
// 2 x 64 x 16 B (f32) of CONTIGUOUS memory instead of 16 rows x 4 KB apart (measured: 3-4 us just to issue
// the uncoalesced loads of a 32-row tile).  Element (m, k) of a [rows][K] matrix sits at frag_idx(m, k, K);
// groups of 8 consecutive k (k % 8 == 0) stay contiguous, so float4 / 8-byte row accesses still work.
Q3_FRAG_FN size_t frag_idx(int m, int k, int K) {
    return ((((size_t)(m >> 4) * (K >> 5) + (k >> 5)) * 64 + (m & 15) + 16 * ((k >> 3) & 3)) << 3) + (k & 7);
}

}  // namespace q3
