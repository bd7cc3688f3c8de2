// q3_timeline.hip -- host control of the diagnostic timeline (the -DQ3_TIMELINE build, lib/libqwen3tts_tl.so); the product
// build keeps only the no-op node numbering.  The state lives here once and is copied to the __device__ instance of every
// translation unit that includes q3_timeline.h (see there).
#include "q3_kernels.h"

#ifndef Q3_TIMELINE
namespace q3 {
int tl_next_node() { return -1; }
}
#endif
#ifdef Q3_TIMELINE
#define Q3_TIMELINE_HOST_ONLY
#include "q3_timeline.h"

namespace q3 {
static TlState g_state;
// the units' refresh functions: filled by their static initialisers, so the list itself must not need one
static int (*g_units[16])(const TlState*);
static int g_n_units = 0;
void tl_register(int (*push)(const TlState*)) {
    if (g_n_units < 16) g_units[g_n_units++] = push;
}
static int tl_push_all() {
    int rc = 0;
    for (int i = 0; i < g_n_units; i++) rc |= g_units[i](&g_state);
    return rc;
}
static int g_tl_node_counter = -1;  // -1: numbering off
int tl_next_node() { return g_tl_node_counter < 0 ? -1 : g_tl_node_counter++; }
int tl2_begin(int max_nodes) {
    if (hipMalloc((void**)&g_state.tl2, (size_t)max_nodes * TL2_MAXB * 16) != hipSuccess) return -1;
    hipMemset(g_state.tl2, 0, (size_t)max_nodes * TL2_MAXB * 16);
    if (hipMalloc((void**)&g_state.tl2_kind, (size_t)max_nodes * 4) != hipSuccess) return -1;
    hipMemset(g_state.tl2_kind, 0xff, (size_t)max_nodes * 4);
    g_state.tl2_nodes = max_nodes;
    if (tl_push_all()) return -1;
    g_tl_node_counter = 0;
    return 0;
}
int tl2_kinds(int* out, int max_nodes) {
    return hipMemcpy(out, g_state.tl2_kind, (size_t)max_nodes * 4, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
int tl2_end(unsigned long long* out, int max_nodes) {
    hipDeviceSynchronize();
    const int n = g_tl_node_counter;
    g_tl_node_counter = -1;
    hipMemcpy(out, g_state.tl2, (size_t)(n < max_nodes ? n : max_nodes) * TL2_MAXB * 16, hipMemcpyDeviceToHost);
    return n;
}
int tl_begin(unsigned cap) {
    unsigned long long* buf = nullptr;
    if (hipMalloc((void**)&buf, (size_t)cap * 16) != hipSuccess) return -1;
    hipMemset(buf, 0, (size_t)cap * 16);
    if (hipMalloc((void**)&g_state.ph, (size_t)cap * 64) != hipSuccess) return -1;
    hipMemset(g_state.ph, 0, (size_t)cap * 64);
    if (!g_state.idx && hipMalloc((void**)&g_state.idx, 4) != hipSuccess) return -1;
    hipMemset(g_state.idx, 0, 4);
    g_state.cap = cap;
    g_state.tl = buf;
    return tl_push_all();
}
int tl_end(unsigned long long* out, unsigned cap) {
    hipDeviceSynchronize();
    unsigned long long* buf = g_state.tl;
    unsigned n = 0;
    if (!buf) return -1;
    hipMemcpy(&n, g_state.idx, 4, hipMemcpyDeviceToHost);
    if (n > cap) n = cap;
    hipMemcpy(out, buf, (size_t)n * 16, hipMemcpyDeviceToHost);
    g_state.tl = nullptr;
    tl_push_all();
    hipFree(buf);
    return (int)n;
}
}  // namespace q3
extern "C" int q3t_set_skip(int on) {
    q3::g_state.skip = on;
    return q3::tl_push_all();
}
extern "C" int q3t_tl_begin(unsigned cap) { return q3::tl_begin(cap); }
extern "C" int q3t_tl_end(unsigned long long* out, unsigned cap) { return q3::tl_end(out, cap); }
extern "C" int q3t_tl2_begin(int max_nodes) { return q3::tl2_begin(max_nodes); }
extern "C" int q3t_tl2_end(unsigned long long* out, int max_nodes) { return q3::tl2_end(out, max_nodes); }
extern "C" int q3t_tl2_kinds(int* out, int max_nodes) { return q3::tl2_kinds(out, max_nodes); }
extern "C" int q3t_tl_phases(unsigned long long* out, unsigned n) {
    return hipMemcpy(out, q3::g_state.ph, (size_t)n * 64, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif
