// q3_voc_settings.h -- the vocoder's run-time settings: one value type, one process-wide store.  Host only (a plain C++ program
// compiles it: tests/voc_settings_host_driver.cpp).
//
// The voc_set_* entry points write the store, from any thread.  An entry point that launches kernels loads it ONCE, into its
// handle (voc_enter, enc_enter, spk_enter), and everything below the entry point -- planning, the walks, the launchers of
// q3_voc_kernels.hip, the overflow check -- reads that snapshot: a call in flight finishes under the settings it started with.
#pragma once
#include <atomic>

namespace q3 {

struct VocSettings {
    int split = 1;       // 1 (default): split-precision fp16 MFMA path where Cin % 16 == 0; 0: exact-fp32 MFMA everywhere
    int fuse = 1;        // 1 (default): residual units at 96 / 192 channels run fused on the exact path
    int max_wgs = 0;     // 0 = one workgroup per tile; >0 caps the grid (persistent tile loop)
    // test hooks (voc_set_fill, voc_set_narrow_k1)
    int fill = -1;       // < 0: the built-in workgroup target of the tile-height rules (512); >= 0 replaces it
    int narrow_k1 = 1;   // 128-column tiles (three workgroups per CU) for the 1-tap convs
};

class VocSettingsStore {
public:
    // (relaxed: the fields are independent, and nothing else is published through them)
    VocSettings load() const {
        VocSettings c;
        c.split = split_.load(std::memory_order_relaxed);
        c.fuse = fuse_.load(std::memory_order_relaxed);
        c.max_wgs = max_wgs_.load(std::memory_order_relaxed);
        c.fill = fill_.load(std::memory_order_relaxed);
        c.narrow_k1 = narrow_k1_.load(std::memory_order_relaxed);
        return c;
    }
    // each -> the value stored
    int set_exact_fp32(int on) { return put(split_, on ? 0 : 1); }
    int set_fused_units(int on) { return put(fuse_, on ? 1 : 0); }
    int set_max_workgroups(int n) { return put(max_wgs_, n); }   // (n < 0, one per compute unit, is resolved by the caller)
    int set_fill(int n) { return put(fill_, n < 0 ? -1 : n); }
    int set_narrow_k1(int on) { return put(narrow_k1_, on ? 1 : 0); }

private:
    static int put(std::atomic<int>& a, int v) {
        a.store(v, std::memory_order_relaxed);
        return v;
    }
    std::atomic<int> split_{VocSettings().split}, fuse_{VocSettings().fuse}, max_wgs_{VocSettings().max_wgs}, fill_{VocSettings().fill},
        narrow_k1_{VocSettings().narrow_k1};
};

extern VocSettingsStore voc_settings;   // the one instance (q3_voc.hip, beside voc_set_exact_fp32)

}  // namespace q3
