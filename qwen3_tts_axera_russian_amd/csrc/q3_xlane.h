// q3_xlane.h -- the cross-lane exchange helpers and the butterflies built on them (device code; the reductions of
// q3_linear.hip, q3_attn.hip, q3_sample.hip, q3_rows.hip and the speaker encoder's, q3_spk.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace q3 {

// ---- cross-lane exchange: the value of lane (l ^ MASK) inside aligned groups of WIDTH lanes ----
// __shfl_xor becomes a ds_bpermute_b32 on gfx950: an LDS instruction, queued behind whatever else the CU's LDS pipe is
// serving (beside the vocoder's persistent workgroups: their ds_reads), its result behind an s_waitcnt lgkmcnt.  The same
// xor butterfly exists in the register file: DPP modifiers inside a row of 16 lanes (the compiler folds the move into the
// add), v_permlane16_swap / v_permlane32_swap across rows.  The exchange is the same, so every reduction built on it
// keeps its tree and its bits.
//
// CONTRACT: every lane of the exchange group (the WIDTH aligned lanes) is active at the call.  A DPP read of an inactive
// lane returns 0 (bound_ctrl), a permlane swap leaves inactive lanes unswapped -- neither is what ds_bpermute returns.
// Uniform-per-group divergence is fine (attn_kernel's `if (t < T)` per 16-lane group with WIDTH 16); a site whose mask
// is not uniform per group keeps __shfl_xor, with a comment saying why (none today; attn_kernel's merge of a wave's
// groups keeps it for another reason, written there).
// -DQ3_XLANE_SHFL (through Q3_EXTRA_HIPCC_FLAGS) expands the helpers to __shfl_xor again: the A/B build, not a runtime knob.
template <int MASK, int WIDTH>
__device__ __forceinline__ int xlane_shfl(int v) {
    return __shfl_xor(v, MASK, WIDTH);
}
template <int CTRL>
__device__ __forceinline__ int dpp_mov(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true);
}
template <int MASK, int WIDTH>
__device__ __forceinline__ int xlane_xor(int v) {
    static_assert(WIDTH == 4 || WIDTH == 16 || WIDTH == 64, "exchange groups are quads, rows or the wave");
    static_assert(MASK > 0 && MASK < WIDTH && (MASK & (MASK - 1)) == 0, "one xor bit inside the group");
#ifdef Q3_XLANE_SHFL
    return xlane_shfl<MASK, WIDTH>(v);
#else
    if constexpr (MASK == 1) {
        return dpp_mov<0xB1>(v);                       // quad_perm:[1,0,3,2]
    } else if constexpr (MASK == 2) {
        return dpp_mov<0x4E>(v);                       // quad_perm:[2,3,0,1]
    } else if constexpr (MASK == 4) {
        return dpp_mov<0x1B>(dpp_mov<0x141>(v));       // row_half_mirror (xor 7), then quad_perm:[3,2,1,0] (xor 3)
    } else if constexpr (MASK == 8) {
        return dpp_mov<0x128>(v);                      // row_ror:8
    } else if constexpr (MASK == 16) {
        // swap(vdst, src): odd rows of vdst <-> even rows of src.  With both = v: [0] holds the even rows' values in
        // every row pair, [1] the odd rows' -- a lane takes the one that is not its own.
        const auto r = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
        return (int)((__lane_id() & 16) ? r[0] : r[1]);
    } else {
        // the same with the wave's halves: [0] = lanes 0-31's values in both halves, [1] = lanes 32-63's
        const auto r = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
        return (int)((__lane_id() & 32) ? r[0] : r[1]);
    }
#endif
}
template <int MASK, int WIDTH>
__device__ __forceinline__ float xlane_xor(float v) {
    return __int_as_float(xlane_xor<MASK, WIDTH>(__float_as_int(v)));
}
template <int MASK, int WIDTH>
__device__ __forceinline__ float xlane_shfl(float v) {
    return __int_as_float(xlane_shfl<MASK, WIDTH>(__float_as_int(v)));
}
// The butterflies of the call sites, stage order spelled by the name: down = WIDTH/2, ..., 2, 1; up = 1, 2, ..., WIDTH/2.
// XL: the exchange (xlane_xor in the kernels; the test hook also instantiates them on xlane_shfl).
struct XlDpp {
    template <int MASK, int WIDTH, typename T>
    static __device__ __forceinline__ T x(T v) { return xlane_xor<MASK, WIDTH>(v); }
};
struct XlShfl {
    template <int MASK, int WIDTH, typename T>
    static __device__ __forceinline__ T x(T v) { return xlane_shfl<MASK, WIDTH>(v); }
};
template <int WIDTH, int MASK = WIDTH / 2, typename XL = XlDpp>
__device__ __forceinline__ float group_sum_down(float v) {
    v += XL::template x<MASK, WIDTH>(v);
    if constexpr (MASK > 1) v = group_sum_down<WIDTH, MASK / 2, XL>(v);
    return v;
}
// two sums side by side, stage by stage (the attention kernels' pair of scores)
template <int WIDTH, int MASK = WIDTH / 2, typename XL = XlDpp>
__device__ __forceinline__ void group_sum_down2(float& a, float& b) {
    a += XL::template x<MASK, WIDTH>(a);
    b += XL::template x<MASK, WIDTH>(b);
    if constexpr (MASK > 1) group_sum_down2<WIDTH, MASK / 2, XL>(a, b);
}
template <int WIDTH, int MASK = 1, typename XL = XlDpp>
__device__ __forceinline__ float group_sum_up(float v) {
    v += XL::template x<MASK, WIDTH>(v);
    if constexpr (MASK * 2 < WIDTH) v = group_sum_up<WIDTH, MASK * 2, XL>(v);
    return v;
}
template <int WIDTH, int MASK = WIDTH / 2, typename XL = XlDpp>
__device__ __forceinline__ float group_max_down(float v) {
    v = fmaxf(v, XL::template x<MASK, WIDTH>(v));
    if constexpr (MASK > 1) v = group_max_down<WIDTH, MASK / 2, XL>(v);
    return v;
}
template <int WIDTH, int MASK = 1, typename XL = XlDpp>
__device__ __forceinline__ float group_max_up(float v) {
    v = fmaxf(v, XL::template x<MASK, WIDTH>(v));
    if constexpr (MASK * 2 < WIDTH) v = group_max_up<WIDTH, MASK * 2, XL>(v);
    return v;
}
// (value, index) arg-max exchange, lowest index wins ties
template <int WIDTH, int MASK = WIDTH / 2, typename XL = XlDpp>
__device__ __forceinline__ void group_argmax_down(float& v, int& idx) {
    const float ov = XL::template x<MASK, WIDTH>(v);
    const int oi = XL::template x<MASK, WIDTH>(idx);
    if (ov > v || (ov == v && oi < idx)) {
        v = ov;
        idx = oi;
    }
    if constexpr (MASK > 1) group_argmax_down<WIDTH, MASK / 2, XL>(v, idx);
}
__device__ __forceinline__ float wave_sum(float v) { return group_sum_down<64>(v); }
__device__ __forceinline__ float wave_max(float v) { return group_max_down<64>(v); }

}  // namespace q3
