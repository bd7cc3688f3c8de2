// voc_settings_host_driver.cpp -- csrc/q3_voc_settings.h in a plain C++ program, built with -fsanitize=thread by
// tests/test_voc_settings_host.py: (a) the defaults and every setter's normalisation, single-threaded; (b) two writers cycling
// every field through a fixed list of legal values against two readers taking 100 000 snapshots each -- every field of every
// snapshot is a member of its list.  Exit 0 / 1 (what failed goes to stderr); a data race is ThreadSanitizer's to report.
#include "q3_voc_settings.h"

#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

using q3::VocSettings;
using q3::VocSettingsStore;

static int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
            failures++;                                                  \
        }                                                                \
    } while (0)

static bool same(const VocSettings& c, int split, int fuse, int max_wgs, int fill, int narrow_k1) {
    return c.split == split && c.fuse == fuse && c.max_wgs == max_wgs && c.fill == fill && c.narrow_k1 == narrow_k1;
}

static void single_threaded() {
    CHECK(same(VocSettings(), 1, 1, 0, -1, 1));
    VocSettingsStore st;
    CHECK(same(st.load(), 1, 1, 0, -1, 1));
    // exact_fp32(on) stores split = !on
    CHECK(st.set_exact_fp32(1) == 0 && same(st.load(), 0, 1, 0, -1, 1));
    CHECK(st.set_exact_fp32(7) == 0 && st.load().split == 0);
    CHECK(st.set_exact_fp32(-1) == 0 && st.load().split == 0);
    CHECK(st.set_exact_fp32(0) == 1 && same(st.load(), 1, 1, 0, -1, 1));
    // fused_units(on) stores on != 0
    CHECK(st.set_fused_units(0) == 0 && same(st.load(), 1, 0, 0, -1, 1));
    CHECK(st.set_fused_units(5) == 1 && st.load().fuse == 1);
    CHECK(st.set_fused_units(-3) == 1 && st.load().fuse == 1);
    // max_workgroups(n) stores n as given (its C entry point resolves n < 0 first)
    CHECK(st.set_max_workgroups(256) == 256 && same(st.load(), 1, 1, 256, -1, 1));
    CHECK(st.set_max_workgroups(8) == 8 && st.load().max_wgs == 8);
    CHECK(st.set_max_workgroups(0) == 0 && st.load().max_wgs == 0);
    // fill(n) stores n >= 0, -1 for every n < 0
    CHECK(st.set_fill(0) == 0 && same(st.load(), 1, 1, 0, 0, 1));
    CHECK(st.set_fill(512) == 512 && st.load().fill == 512);
    CHECK(st.set_fill(-7) == -1 && st.load().fill == -1);
    CHECK(st.set_fill(-1) == -1 && st.load().fill == -1);
    // narrow_k1(on) stores on != 0
    CHECK(st.set_narrow_k1(0) == 0 && same(st.load(), 1, 1, 0, -1, 0));
    CHECK(st.set_narrow_k1(9) == 1 && st.load().narrow_k1 == 1);
    CHECK(same(st.load(), 1, 1, 0, -1, 1));
    // a second store is its own state
    VocSettingsStore other;
    st.set_fill(3);
    CHECK(other.load().fill == -1);
}

// what the writers store, per field (the stored values: after normalisation)
static const std::vector<int> SPLIT = {0, 1}, FUSE = {0, 1}, MAX_WGS = {0, 8, 64, 256}, FILL = {-1, 0, 128, 512}, NARROW = {0, 1};

static bool member(const std::vector<int>& l, int v) {
    for (int x : l)
        if (x == v) return true;
    return false;
}

static void threaded() {
    VocSettingsStore st;
    std::atomic<bool> stop{false};
    std::atomic<long> bad{0};
    auto writer = [&](unsigned phase) {
        for (unsigned i = phase; !stop.load(std::memory_order_relaxed); i++) {
            st.set_exact_fp32(SPLIT[i % SPLIT.size()] ? 0 : 1);
            st.set_fused_units(FUSE[(i / 2) % FUSE.size()]);
            st.set_max_workgroups(MAX_WGS[i % MAX_WGS.size()]);
            st.set_fill(FILL[(i / 3) % FILL.size()]);
            st.set_narrow_k1(NARROW[(i / 5) % NARROW.size()]);
        }
    };
    auto reader = [&]() {
        long b = 0;
        for (int i = 0; i < 100000; i++) {
            const VocSettings c = st.load();
            if (!member(SPLIT, c.split) || !member(FUSE, c.fuse) || !member(MAX_WGS, c.max_wgs) || !member(FILL, c.fill) ||
                !member(NARROW, c.narrow_k1))
                b++;
        }
        bad.fetch_add(b);
    };
    std::thread w0(writer, 0u), w1(writer, 7u), r0(reader), r1(reader);
    r0.join();
    r1.join();
    stop.store(true);
    w0.join();
    w1.join();
    CHECK(bad.load() == 0);
}

int main() {
    single_threaded();
    threaded();
    if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
    return failures ? 1 : 0;
}
