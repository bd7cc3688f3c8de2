// q3_timeline.h -- device side of the diagnostic timeline (only in the -DQ3_TIMELINE build; the product build never
// includes it).  A __device__ variable belongs to one translation unit, so every unit that includes this header has its
// own copy of the state and registers a function that refreshes it; q3_timeline.hip pushes every change to all of them.
#pragma once
#include <hip/hip_runtime.h>

namespace q3 {

struct TlState {
    unsigned long long* tl = nullptr;    // [cap][2] start/end stamps (100 MHz wall clock)
    unsigned int* idx = nullptr;         // the next slot of tl: ONE counter in device memory, shared by every unit's kernels
    unsigned int cap = 0;
    int skip = 0;                        // diagnostic: every kernel returns at once (measures the pure dispatch chain)
    unsigned long long* ph = nullptr;    // [cap][8] phase stamps of block 0 (shader clock)
    unsigned long long* tl2 = nullptr;   // [tl2_nodes][TL2_MAXB][2] per-block start/end stamps
    int tl2_nodes = 0;                   // nodes numbered beyond the buffers are not stamped
    int* tl2_kind = nullptr;             // [nodes] kernel kind id (the Q3_TL id) of each node
};
constexpr int TL2_MAXB = 1024;
void tl_register(int (*push)(const TlState*));   // q3_timeline.hip: the list tl_push_all() walks

#ifndef Q3_TIMELINE_HOST_ONLY   // (q3_timeline.hip itself has no kernel, and so no copy)
static __device__ TlState g_tls;         // this translation unit's copy
static int tl_push_unit(const TlState* s) {
    return hipMemcpyToSymbol(HIP_SYMBOL(g_tls), s, sizeof(*s)) == hipSuccess ? 0 : -1;
}
static const int tl_unit_registered = (tl_register(tl_push_unit), 0);

struct TlScope {
    unsigned int slot = 0xffffffffu;
    int id;
    __device__ __forceinline__ TlScope(int id_) : id(id_) {
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && g_tls.tl) {
            slot = atomicAdd(g_tls.idx, 1u);
            if (slot < g_tls.cap) g_tls.tl[2 * slot] = (wall_clock64() << 8) | (unsigned)id;
        }
    }
    __device__ __forceinline__ ~TlScope() {
        if (slot < g_tls.cap) g_tls.tl[2 * slot + 1] = wall_clock64();
    }
};
struct TlScope2 {
    unsigned long long t0;
    int node, kind;
    __device__ __forceinline__ TlScope2(int n, int k) : node(n), kind(k) { t0 = wall_clock64(); }
    __device__ __forceinline__ ~TlScope2() {
        if (g_tls.tl2 && node >= 0 && node < g_tls.tl2_nodes && threadIdx.x == 0) {
            const unsigned b = blockIdx.x + gridDim.x * blockIdx.y;
            if (b < TL2_MAXB) {
                g_tls.tl2[((size_t)node * TL2_MAXB + b) * 2] = t0;
                g_tls.tl2[((size_t)node * TL2_MAXB + b) * 2 + 1] = wall_clock64();
            }
            if (b == 0 && g_tls.tl2_kind) g_tls.tl2_kind[node] = kind;
        }
    }
};
#endif

}  // namespace q3
