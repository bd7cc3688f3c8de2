// q3_engine.hip -- fused on-device frame loop for B utterances (include/qwen3tts_engine.h).
//
// One frame = [talker_sample -> 16 code-predictor positions (+15 heads/argmax) -> feedback sum ->
// talker step -> final norm -> codec head], captured once per batch size as a hipGraph.  All
// per-utterance state (positions, EOS bookkeeping, emitted codes) lives in device arrays so the
// same graph serves every frame.
#include "../../include/qwen3tts_engine.h"
#include "q3_cp.h"
#include "q3_engine_host.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <memory>
#include <tuple>

using namespace q3;

namespace {

struct Sampling {   // q3e_set_sampling (0 temperature = greedy, the reference's --temperature 0 limit)
    float t_temp = 0.f, t_top_p = 0.95f, c_temp = 0.f;
    int t_top_k = 50, c_top_k = 50;
};
// Everything frame_chain takes from the mutable part of the engine: what a captured frame has baked into its kernel
// arguments.  q3e_run captures again exactly when the state it would launch with differs from the one its graphs hold.
struct FrameState {
    int B = 0, ignore_eos = 0, cap_frames = 0, chains = 0;   // chains: the effective count (the row ranges follow from it)
    int text_cap = 0;
    Sampling smp;
    unsigned long long seed = 0;
    const int* forced = nullptr;         // null: free-running
    const SlotParams* slots = nullptr;   // null outside the per-slot mode, as everything below but the scores
    const float* text_rows = nullptr;
    const int* text_avail = nullptr;
    int* held = nullptr;                 // null unless q3e_text_hold is on
    const SlotRules* rules = nullptr;
    unsigned* seen = nullptr;
    float* scores = nullptr;
    auto key() const {
        return std::tie(B, ignore_eos, cap_frames, chains, text_cap, smp.t_temp, smp.t_top_p, smp.c_temp, smp.t_top_k, smp.c_top_k,
                        seed, forced, slots, text_rows, text_avail, held, rules, seen, scores);
    }
    bool operator==(const FrameState& o) const { return key() == o.key(); }
};
// (no padding: a field added without its place in key() changes the size)
static_assert(sizeof(FrameState) == 10 * 4 + 8 + 8 * sizeof(void*), "FrameState: a new field belongs in key() too");

// The optional features own their memory; the engine holds each through a unique_ptr, null without a reservation.
// Text streamed into running utterances (q3e_text_reserve / q3e_push_text): row f of a text slot's rows is added to the
// feedback of its frame f where the pad stands.  The host writes rows and counters on s between the launches.
struct TextRows {
    DeviceAllocs mem;
    float* rows = nullptr;   // [max_batch][cap][hidden]
    int* avail = nullptr;    // [max_batch] rows pushed (0: not a text slot)
    int* held = nullptr;     // [max_batch] the sampler's per-step verdict, read by the frame's cp_argmax launches
    int cap = 0;
    bool hold = false;       // q3e_text_hold: a starved text slot is held inside the frame while the other rows step on
};
// Per-slot sampler rules (q3e_rules_reserve / q3e_admit_ruled): the rules entry and the set of emitted ids of every slot
struct RuleSets {
    DeviceAllocs mem;
    SlotRules* rules = nullptr;        // [max_batch]
    unsigned* seen = nullptr;          // [max_batch][seen_words]
    int seen_words = 0;                // (cp_vocab + 31) / 32: one bit per audio id
    std::vector<SlotRules> defaults;   // [max_batch], the source of reset_rows' uploads (outlives the stream's copies)
};
// Log-probabilities of the emitted ids (q3e_scores_reserve / q3e_get_scores): one f32 beside every entry of d_codes, written
// by the frame's 16 sampling launches
struct Scores {
    DeviceAllocs mem;
    PinnedAllocs pin;
    float* d = nullptr;   // [max_frames][max_batch][16]
    float* h = nullptr;   // pinned, as large: the scores on their way to the caller
};
// Device pool of the prefix cache (q3e_prefix_cache / q3e_admit_keyed): per entry the KV rows of one prefix and the residual
// row its final norm reads.  Nothing of it is an argument of the captured frame.
struct PrefixPool {
    DeviceAllocs mem;
    half_t* kv = nullptr;     // [entries][layers][2][n_kv][max_rows][128]
    float* state = nullptr;   // [entries][hidden + hidden / 16]
};

struct Engine {
    Model* m = nullptr;
    int max_batch = 0, n_ctx = 0, max_frames = 0;
    hipStream_t s = nullptr;
    KVCache kv_t, kv_c;
    Work wt, wc;  // talker / code-predictor activations
    int prefill_rows = 0;
    // device state: allocated by q3e_create (d_slots and d_forced on first use) and freed with the engine
    DeviceAllocs mem;
    PinnedAllocs pin;
    int *d_slot = nullptr, *d_pos = nullptr;       // prefill row maps [prefill_rows]
    int* d_tiles = nullptr;                        // prefill attention tiles, int[4] each (<= prefill_rows of them)
    int* d_prompt = nullptr;                       // codec prompt of the utterance being admitted, [prefill_rows][16] (q3e_admit_prompted)
    int *d_iota = nullptr;                         // [max_batch]
    int *d_past = nullptr, *d_npast = nullptr, *d_ntext = nullptr, *d_done = nullptr, *d_nframes = nullptr;
    int *d_pos0 = nullptr, *d_posdec = nullptr, *d_lastrow = nullptr;
    int* d_codes = nullptr;  // [max_frames][B][16]
    int* d_forced = nullptr; // [max_frames][B][16] teacher-forced ids (q3e_set_forced_codes)
    bool forced_on = false;
    unsigned long long* d_seed = nullptr;  // [max_batch] draw-stream seed of every slot (device array: graph-safe)
    unsigned long long n_requests = 0, req_seed = 0, n_refills = 0;
    float* d_pad = nullptr;
    // run state
    int B = 0, ignore_eos = 0;
    GraphExec graph[8];   // one captured frame per chain: a single chain replays on s, parallel chains on their cs[c]
    FrameState captured;  // what graph[] was captured with
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float last_run_ms = 0.f, last_prefill_ms = 0.f, last_host_launch_ms = 0.f;
    int* h_done = nullptr;  // pinned [max_batch]
    int* h_read = nullptr;  // pinned [max_batch + max_frames * max_batch * 16]: n_past and the codes on their way to the caller
    Sampling smp;
    unsigned long long seed = 0;
    // independent row groups of one frame run as parallel branches of the graph (latency hiding)
    // (one chain is the default and runs on s: the chain streams and their events exist only once more than one was asked for)
    int n_chains = 1;
    bool use_prio = false;
    int prio_hi = 0;
    hipStream_t cs[8] = {nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[8] = {nullptr};
    // per-slot mode (q3e_open / q3e_admit / q3e_release): every row reads its own budget, sampling settings and draw
    // stream from d_slots; the host's view of every slot -- budget, frames emitted, text rows, steps held -- and every rule
    // over it is the book (q3_engine_host.h)
    bool slot_mode = false;
    SlotParams* d_slots = nullptr;          // [max_batch]
    SlotBook book;
    std::vector<SlotParams> h_sp;           // the slots' device entries (the final push rewrites the flags)
    int up_i[2] = {0, 0};                   // staging of one-word uploads (synchronised before reuse)
    std::unique_ptr<TextRows> text;
    std::unique_ptr<RuleSets> rules;
    std::unique_ptr<Scores> scores;
    std::unique_ptr<PrefixPool> pool;
    // keys and use order of the pool's entries (q3_engine_host.h); it outlives a pool: its counters run on over
    // q3e_prefix_cache, and a keyed admission without a pool is counted as a miss
    PrefixIndex pfx;
    size_t pfx_entry_elems() const { return (size_t)kv_t.n_layers * 2 * kv_t.n_kv * pfx.max_rows() * 128; }

    // The fixed batch counts its frames here, the per-slot batch in the book; the four questions both answer:
    int cap_frames = 0, frames_run = 0;
    int frames_hi = 0;    // frames any slot may have recorded since q3e_start (q3e_refill restarts frames_run, not this)
    bool hold() const { return text && text->hold; }
    // frames recorded so far (per-slot: those of the slot admitted first)
    int frames_recorded() const { return std::min(slot_mode ? book.frames_hi() : frames_hi, max_frames); }
    // frames row b has generated, from its n_past (a prompted slot's began at its prompt's length)
    int generated(int b, int n_past) const { return slot_mode ? book.generated(b, n_past) : n_past; }
    int budget(int b) const { return slot_mode ? book[b].budget : cap_frames; }
    // steps q3e_run may still take (<= 0: none): never past the frames the batch was started for, nor past the codes array
    int room() const { return slot_mode ? book.room(hold(), max_frames) : std::min(cap_frames, max_frames) - frames_run; }
    void advance(int steps) {
        if (slot_mode) return book.advance(steps, hold(), max_frames);
        frames_run += steps;
        frames_hi += steps;
    }

    // chains own contiguous row ranges that must start on a 16-row fragment block
    int chains_eff() const {
        const int nc = n_chains < 1 ? 1 : n_chains;
        return (nc > 1 && B % (16 * nc) == 0) ? nc : 1;
    }
    FrameState frame_state() const {
        FrameState f;
        f.B = B;
        f.ignore_eos = ignore_eos;
        f.cap_frames = cap_frames;
        f.chains = chains_eff();
        f.smp = smp;
        f.seed = seed;
        f.forced = forced_on ? d_forced : nullptr;
        if (slot_mode) {
            f.slots = d_slots;
            if (text) {
                f.text_rows = text->rows;
                f.text_avail = text->avail;
                f.text_cap = text->cap;
                if (text->hold) f.held = text->held;
            }
            if (rules) {
                f.rules = rules->rules;
                f.seen = rules->seen;
            }
        }
        if (scores) f.scores = scores->d;
        return f;
    }
};

// splitmix64 finaliser of (seed + golden * k): the stream derivations of this file
unsigned long long mix_seed(unsigned long long seed, unsigned long long k, unsigned long long golden) {
    unsigned long long z = seed + golden * k;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The talker's final norm into rows row0..row0+R-1 of the post-norm buffers, with the copy that seeds the code predictor's
// position 0 (copy_row_off: where cp_frame expects those rows).  row_map (device, indexed by the output row; null: the
// row itself) names the source rows of the residual stream -- the utterances' last rows after a prefill.
int talker_final_norm(Engine* e, hipStream_t st, int row0, int R, const int* row_map, int copy_row_off) {
    const Model& m = *e->m;
    const int H = m.cfg.hidden;
    FinalNormArgs f;
    f.h = e->wt.h;
    f.ssq = e->wt.ssq;
    f.ssq_parts = H / 16;
    f.gamma = m.talker.final_norm;
    f.eps = m.cfg.eps;
    f.R = R;
    f.row0 = row0;   // output rows (fragment-ordered buffers are indexed, not offset)
    f.H = H;
    f.row_map = row_map;
    f.out_f32 = e->wt.hidden_f32;
    f.out_f16 = e->wt.hidden_f16;
    f.out_copy = e->wc.h;
    f.out_copy_ssq = e->wc.ssq;
    f.out_copy_xh = e->wc.xh;
    f.out_copy_gamma = m.cp.L[0].in_ln;
    f.out_copy_row_off = copy_row_off;
    return launch_final_norm(st, f);
}

// codec head over rows row0..row0+R-1 of the post-norm hidden
int codec_head(Engine* e, hipStream_t st, int row0, int R) {
    const Model& m = *e->m;
    LinArgs a;
    a.wp = m.talker_head.wp;
    a.N = m.cfg.talker_vocab;
    a.K = m.cfg.hidden;
    a.M = row0 + R;
    a.m_begin = row0;
    a.nt = 1;
    a.x16 = e->wt.hidden_f16;
    a.y = e->wt.logits;
    a.ldy = m.cfg.talker_vocab;
    return launch_linear(st, a, PRO_F16, EPI_STORE);
}

// One frame of rows row0..row0+R-1 on st.  Every argument that can change between two runs comes from f (what a capture
// of these launches bakes in, and what q3e_run compares); the rest are the engine's fixed parts -- the model, the work
// areas, the KV caches and the arrays of q3e_create.
int frame_chain(Engine* e, const FrameState& f, hipStream_t st, int row0, int R) {
    const Model& m = *e->m;
    TalkerSampleArgs sa;
    sa.logits = e->wt.logits;
    sa.V = m.cfg.talker_vocab;
    sa.R = R;
    sa.row0 = row0;
    sa.R_total = f.B;
    sa.audio_vocab = m.cfg.cp_vocab;
    sa.eos = m.cfg.codec_eos;
    sa.past = e->d_past;
    sa.n_past = e->d_npast;
    sa.n_text = e->d_ntext;
    sa.done = e->d_done;
    sa.codes = e->d_codes;
    sa.n_frames = e->d_nframes;
    sa.frame_cap = e->max_frames;
    sa.pos0 = e->d_pos0;
    sa.pos = e->d_posdec;
    sa.ignore_eos = f.ignore_eos;
    sa.max_frames = f.cap_frames;
    sa.temperature = f.smp.t_temp;
    sa.top_k = f.smp.t_top_k;
    sa.top_p = f.smp.t_top_p;
    sa.seed = f.seed;
    sa.seed_ptr = e->d_seed;
    sa.forced = f.forced;
    sa.slots = f.slots;
    sa.text_avail = f.held ? f.text_avail : nullptr;   // (the sampler reads the rows' counters only to hold a row)
    sa.held = f.held;
    sa.rules = f.rules;
    sa.seen = f.seen;
    sa.scores = f.scores;
    if (launch_talker_sample(st, sa)) return -1;
    CpFrameIO io;
    io.codes = e->d_codes;
    io.n_frames = e->d_nframes;
    io.frame_cap = e->max_frames;
    io.fb_h = e->wt.h;
    io.fb_ssq = e->wt.ssq;
    io.fb_xh = e->wt.xh;
    io.fb_gamma = m.talker.L[0].in_ln;
    io.pad_embed = e->d_pad;
    io.text_rows = f.text_rows;
    io.text_avail = f.text_avail;
    io.text_cap = f.text_cap;
    io.held = f.held;
    io.temperature = f.smp.c_temp;
    io.top_k = f.smp.c_top_k;
    io.seed = f.seed ^ 0x5851F42D4C957F2Dull;
    io.seed_ptr = e->d_seed;   // (the group index separates the talker's and the code predictor's draws)
    io.forced = f.forced;
    io.slots = f.slots;
    io.rules = f.rules;
    io.scores = f.scores;
    if (cp_frame(st, m, e->wc, e->kv_c, R, io, row0, f.B)) return -1;
    RowMap rm;
    rm.slot_base = 0;        // row r of the batch owns KV slot r (no table: one dependent load less in front of every attention)
    rm.slot_stride = 1;
    rm.pos = e->d_posdec;
    rm.rows_total = f.B;     // a chain of a split batch launches its attention as the whole batch would
    if (run_stack(st, m, m.talker, e->wt, e->kv_t, R, rm, 1024, row0)) return -1;
    return talker_final_norm(e, st, row0, R, nullptr, cp_seed_row0(e->wc, R, row0, f.B)) || codec_head(e, st, row0, R) ? -1 : 0;
}

void chain_rows(const Engine* e, int c, int& row0, int& R) {
    const int nc = e->chains_eff();
    row0 = 0;
    for (int i = 0; i < c; i++) row0 += e->B / nc + (i < e->B % nc ? 1 : 0);
    R = e->B / nc + (c < e->B % nc ? 1 : 0);
}

bool make_stream(const Engine* e, hipStream_t* st) {
    return (e->use_prio ? hipStreamCreateWithPriority(st, hipStreamNonBlocking, e->prio_hi)
                        : hipStreamCreateWithFlags(st, hipStreamNonBlocking)) == hipSuccess;
}

// streams and events of n parallel chains (n > 1 only: a stream that exists occupies a hardware queue of the process)
int ensure_chains(Engine* e, int n) {
    if (n < 2) return 0;
    if (!e->ev_fork) Q3_HIP(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming), -1);
    for (int c = 0; c < n; c++) {
        if (!e->cs[c] && !make_stream(e, &e->cs[c])) return -1;
        if (!e->ev_join[c]) Q3_HIP(hipEventCreateWithFlags(&e->ev_join[c], hipEventDisableTiming), -1);
    }
    return 0;
}

// the stream chain c of the current batch runs on: the engine's own for a single chain
hipStream_t chain_stream(const Engine* e, int c) { return e->chains_eff() == 1 ? e->s : e->cs[c]; }

// one frame of every chain, eagerly, each on its own stream
int frame_eager(Engine* e, const FrameState& f) {
    for (int c = 0; c < f.chains; c++) {
        int row0, R;
        chain_rows(e, c, row0, R);
        if (frame_chain(e, f, chain_stream(e, c), row0, R)) return -1;
    }
    return 0;
}

int fork_chains(Engine* e) {   // chain streams start after everything queued on the main stream (a single chain IS the main stream)
    const int nc = e->chains_eff();
    if (nc == 1) return 0;
    Q3_HIP(hipEventRecord(e->ev_fork, e->s), -1);
    for (int c = 0; c < nc; c++) Q3_HIP(hipStreamWaitEvent(e->cs[c], e->ev_fork, 0), -1);
    return 0;
}
int join_chains(Engine* e) {   // the main stream continues after every chain stream
    const int nc = e->chains_eff();
    if (nc == 1) return 0;
    for (int c = 0; c < nc; c++) {
        Q3_HIP(hipEventRecord(e->ev_join[c], e->cs[c]), -1);
        Q3_HIP(hipStreamWaitEvent(e->s, e->ev_join[c], 0), -1);
    }
    return 0;
}

// body() (-> 0 ok: the launches of a prefill, up to the codec head) between the events behind q3e_last_prefill_ms; the
// stream is synchronised on return
template <class F>
int timed_prefill(Engine* e, F&& body) {
    Q3_HIP(hipEventRecord(e->ev0, e->s), -1);
    if (body()) return -1;
    Q3_HIP(hipEventRecord(e->ev1, e->s), -1);
    Q3_HIP(hipStreamSynchronize(e->s), -1);
    hipEventElapsedTime(&e->last_prefill_ms, e->ev0, e->ev1);
    return 0;
}

}  // namespace

extern "C" {

void q3e_free(void* ee) {
    Engine* e = (Engine*)ee;
    if (!e) return;
    if (e->s) hipStreamSynchronize(e->s);
    for (auto& g : e->graph) g.reset();
    kv_free(e->kv_t);
    kv_free(e->kv_c);
    work_free(e->wt);
    work_free(e->wc);
    for (int c = 0; c < 8; c++) {
        if (e->cs[c]) hipStreamDestroy(e->cs[c]);
        if (e->ev_join[c]) hipEventDestroy(e->ev_join[c]);
    }
    if (e->ev_fork) hipEventDestroy(e->ev_fork);
    if (e->ev0) hipEventDestroy(e->ev0);
    if (e->ev1) hipEventDestroy(e->ev1);
    if (e->s) hipStreamDestroy(e->s);
    if (e->m) model_free(e->m);
    delete e;   // (its owners free the buffers)
}

void* q3e_create(const char* weights, int max_batch, int n_ctx, int max_frames) {
    if (!weights || max_batch <= 0 || n_ctx <= 0 || max_frames <= 0) return nullptr;
    Engine* e = new Engine();
    // the frame loop is a latency-bound dependent chain: its stream gets the highest priority so that its short kernels
    // are placed ahead of throughput work (Q3_STREAM_PRIO=0: the default priority; the vocoder's stream: q3_voc.hip)
    int prio_lo = 0, prio_hi = 0;
    e->use_prio = !(getenv("Q3_STREAM_PRIO") && atoi(getenv("Q3_STREAM_PRIO")) == 0) &&
                  hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) == hipSuccess && prio_lo != prio_hi;
    e->prio_hi = prio_hi;
    // ONE stream: uploads, prefill, the frame graph and the read-backs (the loader borrows it too), so the engine
    // occupies one hardware queue of the process and nothing of it runs on the null stream
    if (!make_stream(e, &e->s)) {
        Q3_LOG("q3e_create: no stream");
        q3e_free(e);
        return nullptr;
    }
    Model* m = model_load(weights, true, true, nullptr, e->s);
    if (!m) {
        q3e_free(e);
        return nullptr;
    }
    e->m = m;
    if (n_ctx > m->max_pos) {
        Q3_LOG("q3e_create: n_ctx=%d exceeds the RoPE table (%d)", n_ctx, m->max_pos);
        q3e_free(e);
        return nullptr;
    }
    e->max_batch = max_batch;
    e->n_ctx = n_ctx;
    e->max_frames = max_frames;
    const ModelCfg& c = m->cfg;
    e->prefill_rows = max_batch > 2048 ? max_batch : 2048;
    bool ok = hipEventCreate(&e->ev0) == hipSuccess && hipEventCreate(&e->ev1) == hipSuccess;
    if (const char* nc = getenv("Q3_CHAINS")) e->n_chains = atoi(nc) < 1 ? 1 : atoi(nc) > 8 ? 8 : atoi(nc);
    else e->n_chains = 1;  // measured on MI355X/ROCm 7.2: graphs on separate streams do not overlap here
    ok = ok && ensure_chains(e, e->n_chains) == 0;
    ok = ok && kv_alloc(e->kv_t, c.talker_layers, max_batch, c.n_kv, n_ctx, e->s) == 0;
    ok = ok && kv_alloc(e->kv_c, c.cp_layers, max_batch, c.n_kv, c.cp_groups + 1, e->s) == 0;
    ok = ok && work_alloc(e->wt, c, e->prefill_rows, c.talker_ffn, c.talker_vocab, e->s) == 0;
    ok = ok && work_alloc(e->wc, c, 2 * ((max_batch + 15) / 16 * 16), c.cp_ffn, c.cp_vocab, e->s) == 0;   // two rows per utterance in the CP's first pass
    const size_t mb = max_batch, pr = e->prefill_rows;
    const std::pair<int**, size_t> ints[] = {
        {&e->d_slot, pr},   {&e->d_pos, pr},   {&e->d_tiles, 4 * pr}, {&e->d_prompt, 16 * pr}, {&e->d_iota, mb},
        {&e->d_past, 32 * mb}, {&e->d_npast, mb}, {&e->d_ntext, mb}, {&e->d_done, mb}, {&e->d_nframes, mb},
        {&e->d_pos0, mb},   {&e->d_posdec, mb}, {&e->d_lastrow, mb},   {&e->d_codes, 16 * mb * max_frames}};
    for (const auto& a : ints) ok = ok && e->mem.alloc(a.first, sizeof(int) * a.second);
    ok = ok && e->mem.alloc_zeroed(&e->d_pad, sizeof(float) * c.hidden, e->s);
    ok = ok && e->mem.alloc_zeroed(&e->d_seed, sizeof(unsigned long long) * mb, e->s);
    ok = ok && e->pin.alloc(&e->h_done, sizeof(int) * mb) && e->pin.alloc(&e->h_read, sizeof(int) * (mb + 16 * mb * max_frames));
    if (ok) {
        std::vector<int> iota(max_batch);
        for (int i = 0; i < max_batch; i++) iota[i] = i;
        ok = hipMemcpyAsync(e->d_iota, iota.data(), sizeof(int) * max_batch, hipMemcpyHostToDevice, e->s) == hipSuccess;
        ok = hipStreamSynchronize(e->s) == hipSuccess && ok;   // (iota is a local)
    }
    if (!ok) {
        Q3_LOG("q3e_create: allocation failed");
        q3e_free(e);
        return nullptr;
    }
    return e;
}

int q3e_set_sampling(void* ee, float talker_temperature, int talker_top_k, float talker_top_p, float cp_temperature,
                     int cp_top_k, uint64_t seed) {
    Engine* e = (Engine*)ee;
    if (!e) return -1;
    e->smp = {talker_temperature, talker_top_p, cp_temperature, talker_top_k, cp_top_k};
    e->seed = seed;
    e->n_requests = 0;
    return 0;
}

int q3e_set_forced_codes(void* ee, const int32_t* forced, int n_frames) {
    Engine* e = (Engine*)ee;
    if (!e) return -1;
    const bool on = forced != nullptr && n_frames > 0;
    if (on && e->slot_mode) {
        Q3_LOG("q3e_set_forced_codes: not for a per-slot batch (q3e_open)");
        return -1;
    }
    if (on) {
        if (e->B <= 0 || n_frames > e->max_frames) return -1;
        const size_t total = (size_t)e->max_frames * e->max_batch * 16;
        if (!e->d_forced && !e->mem.alloc(&e->d_forced, sizeof(int) * total)) {
            Q3_LOG("q3e_set_forced_codes: allocation of %zu bytes failed", sizeof(int) * total);
            return -1;
        }
        Q3_HIP(hipMemsetAsync(e->d_forced, 0xff, sizeof(int) * total, e->s), -1);   // -1 = free-running
        Q3_HIP(hipMemcpyAsync(e->d_forced, forced, sizeof(int) * 16 * (size_t)e->B * n_frames, hipMemcpyHostToDevice, e->s), -1);
        Q3_HIP(hipStreamSynchronize(e->s), -1);   // the caller's array is its own again on return
    }
    e->forced_on = on;
    return 0;
}

int q3e_set_chains(void* ee, int n) {
    Engine* e = (Engine*)ee;
    if (!e || n < 1 || n > 8) return -1;
    if (n != e->n_chains) {
        if (ensure_chains(e, n)) return -1;
        e->n_chains = n;
    }
    return 0;
}

int q3e_set_pad_embed(void* ee, const float* pad) {
    Engine* e = (Engine*)ee;
    if (!e || !pad) return -1;
    Q3_HIP(hipMemcpyAsync(e->d_pad, pad, sizeof(float) * e->m->cfg.hidden, hipMemcpyHostToDevice, e->s), -1);
    Q3_HIP(hipStreamSynchronize(e->s), -1);
    return 0;
}

// Final norm after a prefill: the rows d_lastrow[row0 .. row0 + R) of the residual stream into rows row0.. of the post-norm
// buffers and of the code predictor's position-0 input (prefill_ids; a prefix-cache hit launches it for its one row)
static int prefill_final_norm(Engine* e, int row0, int R, int B_total) {
    // the first frame's code predictor pass reads its position-0 rows where cp_frame expects them (the same
    // place for one chain and for parallel chains)
    return talker_final_norm(e, e->s, row0, R, e->d_lastrow, cp_seed_row0(e->wc, B_total, 0, B_total));
}

// The codec prompt in d_prompt (T frames) into slot `slot`: its sampler state, and with `rows` its T talker rows into rows
// row0.. of the talker's residual stream, as launch_ssq_rows leaves uploaded rows (launch_prompt_rows)
static int prompt_launch(Engine* e, int slot, int T, int row0, bool rows) {
    const Model& m = *e->m;
    PromptRowsArgs a;
    a.codes = e->d_prompt;
    a.T = T;
    a.past = e->d_past + 32 * (size_t)slot;
    a.n_past = e->d_npast + slot;
    a.talker_emb = m.talker_emb;
    a.talker_vocab = m.cfg.talker_vocab;
    a.cp_tables = m.d_cp_emb_ptrs;
    a.cp_vocab = m.cfg.cp_vocab;
    a.n_groups = m.cfg.cp_groups;
    a.pad_embed = e->d_pad;
    if (e->rules) {   // (reset_rows has cleared the slot's set)
        a.seen = e->rules->seen + (size_t)(slot < 0 ? 0 : slot) * e->rules->seen_words;
        a.seen_vocab = m.cfg.cp_vocab;   // (the sampler's audio_vocab, frame_chain)
    }
    if (rows) {
        a.h = e->wt.h;
        a.ssq = e->wt.ssq;
        a.xh = e->wt.xh;
        a.gamma = m.talker.L[0].in_ln;
        a.row0 = row0;
        a.max_rows = e->prefill_rows;
        a.H = m.cfg.hidden;
    }
    if (slot < 0 || slot >= e->max_batch || T > e->prefill_rows) return -1;
    return launch_prompt_rows(e->s, a);
}

// Ragged prefill of n utterances into the KV slots / output rows ids[0..n) (prefix rows concatenated in that order):
// utterances are packed into passes of at most prefill_rows rows; every row carries its own (slot, position).  The
// hidden of each utterance's last row lands in row ids[u] of the post-norm buffers, one group at a time.
// n_prompt > 0 (n == 1 only): the last n_prompt of the utterance's n_rows[0] rows are not in `prefix`; they are built on
// the device from the codec prompt in d_prompt, which also seeds the slot's sampler state.
static int prefill_ids(Engine* e, int n, const int* ids, const float* prefix, const int32_t* n_rows, int B_total, int n_prompt = 0) {
    if (n_prompt && (n != 1 || n_prompt >= n_rows[0])) return -1;
    const Model& m = *e->m;
    const int H = m.cfg.hidden;
    size_t row_off = 0;
    int u0 = 0;
    std::vector<int> slot, pos, tiles, last(n);
    while (u0 < n) {
        int u1 = u0, rows = 0;
        while (u1 < n && rows + n_rows[u1] <= e->prefill_rows) rows += n_rows[u1++];
        slot.resize(rows);
        pos.resize(rows);
        int r = 0;
        tiles.clear();
        bool contiguous = true;
        for (int u = u0; u < u1; u++) {
            const int b = ids[u];
            if (u > u0 && b != ids[u - 1] + 1) contiguous = false;
            for (int i = 0; i < n_rows[u]; i += 16) {      // the utterance's rows as runs of <= 16 positions (attn_tile_kernel)
                const int nn = n_rows[u] - i < 16 ? n_rows[u] - i : 16;
                const int t4[4] = {r + i, nn, b, i};
                tiles.insert(tiles.end(), t4, t4 + 4);
            }
            for (int i = 0; i < n_rows[u]; i++, r++) {
                slot[r] = b;
                pos[r] = i;
            }
            last[u] = r - 1;
        }
        const int up_rows = rows - n_prompt;   // rows that come from the host
        Q3_HIP(hipMemcpyAsync(e->wt.rows_in, prefix + row_off * H, sizeof(float) * (size_t)up_rows * H, hipMemcpyHostToDevice, e->s), -1);
        Q3_HIP(hipMemcpyAsync(e->d_slot, slot.data(), sizeof(int) * rows, hipMemcpyHostToDevice, e->s), -1);
        Q3_HIP(hipMemcpyAsync(e->d_pos, pos.data(), sizeof(int) * rows, hipMemcpyHostToDevice, e->s), -1);
        Q3_HIP(hipMemcpyAsync(e->d_tiles, tiles.data(), sizeof(int) * tiles.size(), hipMemcpyHostToDevice, e->s), -1);
        if (contiguous) {
            Q3_HIP(hipMemcpyAsync(e->d_lastrow + ids[u0], last.data() + u0, sizeof(int) * (u1 - u0), hipMemcpyHostToDevice, e->s), -1);
        } else {
            for (int u = u0; u < u1; u++)
                Q3_HIP(hipMemcpyAsync(e->d_lastrow + ids[u], last.data() + u, sizeof(int), hipMemcpyHostToDevice, e->s), -1);
        }
        if (launch_ssq_rows(e->s, e->wt.rows_in, e->wt.h, e->wt.ssq, up_rows, H, e->wt.xh, m.talker.L[0].in_ln)) return -1;
        if (n_prompt && prompt_launch(e, ids[u0], n_prompt, up_rows, true)) return -1;
        RowMap rm;
        rm.slot = e->d_slot;
        rm.pos = e->d_pos;
        rm.same_slot_rows = true;
        rm.tiles = e->d_tiles;
        rm.n_tiles = (int)(tiles.size() / 4);
        if (run_stack(e->s, m, m.talker, e->wt, e->kv_t, rows, rm, 1024)) return -1;
        // final norm of the last rows of this group into rows ids[u0..u1) of the post-norm buffers
        for (int u = u0; u < u1; u += contiguous ? (u1 - u0) : 1)
            if (prefill_final_norm(e, ids[u], contiguous ? u1 - u0 : 1, B_total)) return -1;
        Q3_HIP(hipStreamSynchronize(e->s), -1);  // host staging vectors are reused by the next group
        row_off += rows;
        u0 = u1;
    }
    return 0;
}

// the columns of rows b0..b0+n-1 in every frame of a [max_frames][B][16] array of 4-byte entries, filled with byte v
static int fill_columns(Engine* e, void* a, int b0, int n, int v) {
    const size_t pitch = 4 * 16 * (size_t)e->B;
    if (n == e->B) Q3_HIP(hipMemsetAsync(a, v, pitch * e->max_frames, e->s), -1);
    else Q3_HIP(hipMemset2DAsync((char*)a + 4 * 16 * (size_t)b0, pitch, v, 4 * 16 * (size_t)n, e->max_frames, e->s), -1);
    return 0;
}

// Rows b0..b0+n-1 of every per-slot device array back to a start state, asynchronously on e->s:
//   fresh  "just started": counters 0, an empty emitted-token ring, positions n_rows[0..n), text lengths n_text[0..n) (null:
//          0 -- a text slot's comes with its final push); host arrays that must live until the stream is synchronised
//   idle   ended (done) with the frame counter at the end of the codes array, so nothing is recorded, at position 0
// and either way the rows' columns of the codes array to -1 and no text row pushed, no hold; under q3e_rules_reserve an empty
// seen-set and default rules: a recycled slot inherits neither the previous utterance's history nor its rules.
enum class RowStart { fresh, idle };
static int reset_rows(Engine* e, int b0, int n, RowStart how, const int32_t* n_rows = nullptr, const int32_t* n_text = nullptr) {
    const bool idle = how == RowStart::idle;
    const size_t bytes = sizeof(int) * n;
    Q3_HIP(hipMemsetAsync(e->d_npast + b0, 0, bytes, e->s), -1);
    Q3_HIP(hipMemsetD32Async((hipDeviceptr_t)(e->d_done + b0), idle ? 1 : 0, n, e->s), -1);
    Q3_HIP(hipMemsetD32Async((hipDeviceptr_t)(e->d_nframes + b0), idle ? e->max_frames : 0, n, e->s), -1);
    Q3_HIP(hipMemsetAsync(e->d_past + 32 * b0, 0, 32 * bytes, e->s), -1);
    if (fill_columns(e, e->d_codes, b0, n, 0xff)) return -1;
    // the rows' columns of the scores, zeroed wherever their codes are reset
    if (e->scores && fill_columns(e, e->scores->d, b0, n, 0)) return -1;
    if (idle || !n_text) Q3_HIP(hipMemsetAsync(e->d_ntext + b0, 0, bytes, e->s), -1);
    else Q3_HIP(hipMemcpyAsync(e->d_ntext + b0, n_text, bytes, hipMemcpyHostToDevice, e->s), -1);
    if (idle) {
        Q3_HIP(hipMemsetAsync(e->d_pos0 + b0, 0, bytes, e->s), -1);
        Q3_HIP(hipMemsetAsync(e->d_posdec + b0, 0, bytes, e->s), -1);
        Q3_HIP(hipMemsetAsync(e->d_lastrow + b0, 0, bytes, e->s), -1);
    } else {
        Q3_HIP(hipMemcpyAsync(e->d_pos0 + b0, n_rows, bytes, hipMemcpyHostToDevice, e->s), -1);
        Q3_HIP(hipMemcpyAsync(e->d_posdec + b0, n_rows, bytes, hipMemcpyHostToDevice, e->s), -1);
    }
    if (e->text) {
        Q3_HIP(hipMemsetAsync(e->text->avail + b0, 0, bytes, e->s), -1);
        Q3_HIP(hipMemsetAsync(e->text->held + b0, 0, bytes, e->s), -1);
    }
    if (const RuleSets* r = e->rules.get()) {
        Q3_HIP(hipMemsetAsync(r->seen + (size_t)b0 * r->seen_words, 0, sizeof(unsigned) * (size_t)n * r->seen_words, e->s), -1);
        Q3_HIP(hipMemcpyAsync(r->rules + b0, r->defaults.data(), sizeof(SlotRules) * n, hipMemcpyHostToDevice, e->s), -1);
    }
    return 0;
}

// codec head over rows 0..B-1 of the post-norm hidden (rows of running utterances give the logits they already have)
static int head_all_rows(Engine* e) { return codec_head(e, e->s, 0, e->B); }

// n_rows prefix rows and `frames` frames of utterance u fit a prefill pass and the context
static bool check_fit(const Engine* e, const char* who, int u, int n_rows, int frames) {
    if (n_rows > 0 && n_rows <= e->prefill_rows && n_rows + frames <= e->n_ctx) return true;
    Q3_LOG("%s: utterance %d: %d prefix rows + %d frames do not fit n_ctx=%d", who, u, n_rows, frames, e->n_ctx);
    return false;
}

// slots[u] is one of the batch's B and none of slots[0..u) (called for u = 0, 1, ..: a list is checked in its order,
// between the other checks of each utterance)
static bool check_slot_list(const char* who, int u, const int32_t* slots, int B) {
    if (slots[u] >= 0 && slots[u] < B && std::find(slots, slots + u, slots[u]) == slots + u) return true;
    Q3_LOG("%s: slot %d is out of range or listed twice (batch of %d)", who, slots[u], B);
    return false;
}

int q3e_start(void* ee, int B, const float* prefix, const int32_t* n_rows, const int32_t* n_text, int ignore_eos,
              int max_frames) {
    Engine* e = (Engine*)ee;
    if (!e || !prefix || !n_rows || !n_text || B <= 0 || B > e->max_batch) return -1;
    if (max_frames <= 0 || max_frames > e->max_frames) max_frames = e->max_frames;
    for (int b = 0; b < B; b++)
        if (!check_fit(e, "q3e_start", b, n_rows[b], max_frames)) return -1;
    e->B = B;
    e->ignore_eos = ignore_eos ? 1 : 0;
    e->cap_frames = max_frames;
    e->frames_run = 0;
    e->frames_hi = 0;
    e->slot_mode = false;
    if (reset_rows(e, 0, B, RowStart::fresh, n_rows, n_text)) return -1;
    // a fresh draw stream per request (the reference's generators advance from their seed across requests); the row
    // index separates the slots' draws
    const unsigned long long k = e->n_requests++;
    e->req_seed = k == 0 ? e->seed : mix_seed(e->seed, k, 0x9E3779B97F4A7C15ull);
    e->n_refills = 0;
    const std::vector<unsigned long long> seeds(B, e->req_seed);   // (alive until the stream is synchronised)
    Q3_HIP(hipMemcpyAsync(e->d_seed, seeds.data(), sizeof(unsigned long long) * B, hipMemcpyHostToDevice, e->s), -1);
    e->forced_on = false;   // forcing belongs to the batch it was set for
    Q3_HIP(hipStreamSynchronize(e->s), -1);
    std::vector<int> ids(B);
    for (int b = 0; b < B; b++) ids[b] = b;
    return timed_prefill(e, [&] { return prefill_ids(e, B, ids.data(), prefix, n_rows, B) || head_all_rows(e); });
}

int q3e_run(void* ee, int n_frames) {
    Engine* e = (Engine*)ee;
    if (!e || e->B <= 0 || n_frames <= 0) return -1;
    n_frames = std::min(n_frames, e->room());
    if (n_frames <= 0) return 0;
    int done_frames = 0;
    const FrameState cur = e->frame_state();
    const int nc = cur.chains;
    Q3_HIP(hipEventRecord(e->ev0, e->s), -1);
    if (fork_chains(e)) return -1;
    // Q3_NO_GRAPH=1: eager launches (rocprofv3 --kernel-trace crashes on the graph replay)
    static const bool no_graph = getenv("Q3_NO_GRAPH") && atoi(getenv("Q3_NO_GRAPH")) != 0;
    if (no_graph) {
        for (; done_frames < n_frames; done_frames++)
            if (frame_eager(e, cur)) return -1;
    } else if (!e->graph[0].e || !(cur == e->captured)) {
        // first frame eagerly (real work; also sets the kernels' LDS attributes), then capture per chain
        if (frame_eager(e, cur)) return -1;
        done_frames++;
        for (int c = 0; c < nc; c++) Q3_HIP(hipStreamSynchronize(chain_stream(e, c)), -1);
        e->captured = FrameState();   // (B = 0, no state of a run: a capture that fails half way leaves no graph to replay)
        for (int c = 0; c < nc; c++) {
            int row0, R;
            chain_rows(e, c, row0, R);
            hipStream_t st = chain_stream(e, c);
            if (e->graph[c].capture(st, hipStreamCaptureModeRelaxed, "q3e_run", [&] { return frame_chain(e, cur, st, row0, R); }))
                return -1;
        }
        e->captured = cur;
    }
    const int check_every = 16;
    const auto th0 = std::chrono::steady_clock::now();
    while (!no_graph && done_frames < n_frames) {
        int chunk = n_frames - done_frames;
        if (!e->ignore_eos && chunk > check_every) chunk = check_every;
        for (int i = 0; i < chunk; i++)
            for (int c = 0; c < nc; c++) Q3_HIP(hipGraphLaunch(e->graph[c].e, chain_stream(e, c)), -1);
        done_frames += chunk;
        if (!e->ignore_eos && done_frames < n_frames) {
            if (join_chains(e)) return -1;
            Q3_HIP(hipMemcpyAsync(e->h_done, e->d_done, sizeof(int) * e->B, hipMemcpyDeviceToHost, e->s), -1);
            Q3_HIP(hipStreamSynchronize(e->s), -1);
            bool all = true;
            for (int b = 0; b < e->B; b++) all = all && e->h_done[b];
            if (all) break;
            if (fork_chains(e)) return -1;
        }
    }
    e->last_host_launch_ms = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - th0).count();
    if (join_chains(e)) return -1;
    Q3_HIP(hipEventRecord(e->ev1, e->s), -1);
    Q3_HIP(hipStreamSynchronize(e->s), -1);
    hipEventElapsedTime(&e->last_run_ms, e->ev0, e->ev1);
    e->advance(done_frames);
    return done_frames;
}

int q3e_graph_nodes(void* ee) {
    Engine* e = (Engine*)ee;
    if (!e) return -1;
    if (!e->graph[0].g) return 0;
    size_t n = 0;
    Q3_HIP(hipGraphGetNodes(e->graph[0].g, nullptr, &n), -1);
    return (int)n;
}

float q3e_last_run_ms(void* ee) { return ee ? ((Engine*)ee)->last_run_ms : -1.f; }
float q3e_last_host_launch_ms(void* ee) { return ee ? ((Engine*)ee)->last_host_launch_ms : -1.f; }
float q3e_last_prefill_ms(void* ee) { return ee ? ((Engine*)ee)->last_prefill_ms : -1.f; }

// The getters' read-back: n_past of the batch's rows into h_read[0..B) and, as asked, the first nf recorded frames (at most
// max_out) of the codes behind them (h_read + max_batch) and of the scores into their pinned buffer, on the engine's own
// stream (a pageable destination would go through the runtime's staging), synchronised on return.  -> nf, < 0 on error
static int read_back(Engine* e, int max_out, bool codes, bool scores) {
    const int nf = std::min(e->frames_recorded(), max_out);
    const size_t n = 16 * (size_t)e->B * (nf > 0 ? nf : 0);
    Q3_HIP(hipMemcpyAsync(e->h_read, e->d_npast, sizeof(int) * e->B, hipMemcpyDeviceToHost, e->s), -1);
    if (codes && n) Q3_HIP(hipMemcpyAsync(e->h_read + e->max_batch, e->d_codes, sizeof(int) * n, hipMemcpyDeviceToHost, e->s), -1);
    if (scores && n) Q3_HIP(hipMemcpyAsync(e->scores->h, e->scores->d, sizeof(float) * n, hipMemcpyDeviceToHost, e->s), -1);
    Q3_HIP(hipStreamSynchronize(e->s), -1);
    return nf;
}

int q3e_get_codes(void* ee, int32_t* out, int max_out_frames, int32_t* n_frames_per_utt) {
    Engine* e = (Engine*)ee;
    if (!e || !out || e->B <= 0) return -1;
    const int nf = read_back(e, max_out_frames, true, false);
    if (nf < 0) return nf;
    memcpy(out, e->h_read + e->max_batch, sizeof(int) * 16 * (size_t)e->B * nf);
    if (n_frames_per_utt)
        for (int b = 0; b < e->B; b++) n_frames_per_utt[b] = e->generated(b, e->h_read[b]);
    return nf;
}

int q3e_scores_reserve(void* ee, int on) {
    Engine* e = (Engine*)ee;
    if (!e) return -1;
    if (e->slot_mode) {
        Q3_LOG("q3e_scores_reserve: a per-slot batch is open (call before q3e_open)");
        return -1;
    }
    Q3_HIP(hipStreamSynchronize(e->s), -1);
    if ((on != 0) == (e->scores != nullptr)) return 0;
    e->scores.reset();
    if (!on) return 0;
    auto sc = std::make_unique<Scores>();
    const size_t bytes = sizeof(float) * 16 * (size_t)e->max_frames * e->max_batch;
    if (!sc->mem.alloc_zeroed(&sc->d, bytes, e->s) || !sc->pin.alloc(&sc->h, bytes)) {
        Q3_LOG("q3e_scores_reserve: allocation of %zu bytes failed", bytes);
        return -1;
    }
    Q3_HIP(hipStreamSynchronize(e->s), -1);
    e->scores = std::move(sc);
    return 0;
}

int q3e_get_scores(void* ee, float* out, int max_out_frames, int32_t* n_frames_per_utt) {
    Engine* e = (Engine*)ee;
    if (!e || !out || e->B <= 0) return -1;
    if (!e->scores) {
        Q3_LOG("q3e_get_scores: no scores are reserved (q3e_scores_reserve)");
        return -1;
    }
    const int nf = read_back(e, max_out_frames, true, true);   // (the frames of q3e_get_codes)
    if (nf < 0) return nf;
    const int* h_codes = e->h_read + e->max_batch;
    // what the kernels leave for a row that has ended is unspecified: a frame without a code_0 (column 0 < 0), and every
    // frame at or past the utterance's count, reads 0
    for (int f = 0; f < nf; f++)
        for (int b = 0; b < e->B; b++) {
            const size_t at = ((size_t)f * e->B + b) * 16;
            const bool live = h_codes[at] >= 0 && f < e->generated(b, e->h_read[b]);
            for (int g = 0; g < 16; g++) out[at + g] = live ? e->scores->h[at + g] : 0.f;
        }
    if (n_frames_per_utt)
        for (int b = 0; b < e->B; b++) n_frames_per_utt[b] = e->generated(b, e->h_read[b]);
    return nf;
}

int q3e_get_done(void* ee, int32_t* done, int32_t* frames) {
    Engine* e = (Engine*)ee;
    if (!e || !done || e->B <= 0) return -1;
    Q3_HIP(hipMemcpyAsync(e->h_done, e->d_done, sizeof(int) * e->B, hipMemcpyDeviceToHost, e->s), -1);
    if (read_back(e, 0, false, false) < 0) return -1;
    memcpy(done, e->h_done, sizeof(int) * e->B);
    // the device raises done[b] on the step AFTER the budget's last frame, a step q3e_run never takes: an utterance
    // that has emitted its whole budget has ended
    for (int b = 0; b < e->B; b++) {
        const int generated = e->generated(b, e->h_read[b]);
        if (generated >= e->budget(b)) done[b] = 1;
        if (e->slot_mode && done[b]) e->book.mark_ended(b);
        if (frames) frames[b] = generated;
    }
    return 0;
}

int q3e_refill(void* ee, int n, const int32_t* slots, const float* prefix, const int32_t* n_rows, const int32_t* n_text) {
    Engine* e = (Engine*)ee;
    if (!e || e->B <= 0 || n <= 0 || n > e->B || !slots || !prefix || !n_rows || !n_text) return -1;
    if (e->forced_on) {
        Q3_LOG("q3e_refill: a teacher-forced batch cannot be refilled");
        return -1;
    }
    if (e->slot_mode) {
        Q3_LOG("q3e_refill: a per-slot batch (q3e_open) takes new utterances with q3e_admit");
        return -1;
    }
    for (int u = 0; u < n; u++)
        if (!check_slot_list("q3e_refill", u, slots, e->B) || !check_fit(e, "q3e_refill", u, n_rows[u], e->cap_frames)) return -1;
    Q3_HIP(hipStreamSynchronize(e->s), -1);
    std::vector<unsigned long long> seeds(n);   // (alive until timed_prefill has synchronised the stream)
    const int rc = timed_prefill(e, [&]() -> int {
        for (int u = 0; u < n; u++) {
            if (reset_rows(e, slots[u], 1, RowStart::fresh, n_rows + u, n_text + u)) return -1;
            // a fresh draw stream for the new occupant: the counters (frame, group) restart with the slot, so keeping the
            // request's seed would replay the previous occupant's uniforms
            seeds[u] = mix_seed(e->req_seed, ++e->n_refills, 0xD1B54A32D192ED03ull);
            Q3_HIP(hipMemcpyAsync(e->d_seed + slots[u], &seeds[u], sizeof(seeds[u]), hipMemcpyHostToDevice, e->s), -1);
        }
        Q3_HIP(hipStreamSynchronize(e->s), -1);
        return prefill_ids(e, n, slots, prefix, n_rows, e->B) || head_all_rows(e);
    });
    if (rc) return -1;
    e->frames_run = 0;   // the new utterances have their whole frame budget; running ones stop at theirs on the device
    return 0;
}

int q3e_open(void* ee, int B, int ignore_eos) {
    Engine* e = (Engine*)ee;
    if (!e || B <= 0 || B > e->max_batch) return -1;
    const Model& m = *e->m;
    const ModelCfg& c = m.cfg;
    if (c.talker_vocab > 4096 || c.cp_vocab > 4096) {   // SAMPLE_SORT_CAP: every row may take the sort path
        Q3_LOG("q3e_open: vocabularies of %d / %d are beyond the per-slot sampler", c.talker_vocab, c.cp_vocab);
        return -1;
    }
    Q3_HIP(hipStreamSynchronize(e->s), -1);
    if (!e->d_slots && !e->mem.alloc(&e->d_slots, sizeof(SlotParams) * e->max_batch)) {
        Q3_LOG("q3e_open: allocation failed");
        return -1;
    }
    e->B = B;
    e->ignore_eos = ignore_eos ? 1 : 0;
    e->cap_frames = e->max_frames;
    e->frames_run = 0;
    e->frames_hi = 0;
    e->slot_mode = true;
    e->book.open(B);
    e->h_sp.assign(B, SlotParams());
    e->forced_on = false;
    // idle rows step through the graph with everything else: they have ended (done), their frame counter sits at the end of
    // the codes array (nothing is recorded), and they run at position 0 of zeroed caches and activations (finite values;
    // rows are independent, so what an idle row computes never reaches another row)
    if (reset_rows(e, 0, B, RowStart::idle)) return -1;
    Q3_HIP(hipMemsetAsync(e->d_slots, 0, sizeof(SlotParams) * e->max_batch, e->s), -1);
    if (kv_zero(e->s, e->kv_t) || kv_zero(e->s, e->kv_c)) return -1;
    if (work_zero(e->s, e->wt, c, c.talker_ffn, c.talker_vocab) || work_zero(e->s, e->wc, c, c.cp_ffn, c.cp_vocab)) return -1;
    Q3_HIP(hipStreamSynchronize(e->s), -1);
    return 0;
}

// one utterance's prefix state between its slot and pool entry i (launch_prefix_move); h_row: the row of the talker's
// residual stream the state sits in
static int prefix_move(Engine* e, int i, int slot, int n_rows, int h_row, int restore) {
    PrefixMoveArgs a;
    a.kc = e->kv_t.k;
    a.vc = e->kv_t.v;
    a.layer_stride = e->kv_t.layer_stride();
    a.n_layers = e->kv_t.n_layers;
    a.n_kv = e->kv_t.n_kv;
    a.n_ctx = e->kv_t.n_ctx;
    a.slot = slot;
    a.n_rows = n_rows;
    a.entry = e->pool->kv + (size_t)i * e->pfx_entry_elems();
    a.max_rows = e->pfx.max_rows();
    const int H = e->m->cfg.hidden;
    a.state = e->pool->state + (size_t)i * (H + H / 16);
    a.h = e->wt.h;
    a.ssq = e->wt.ssq;
    a.h_row = h_row;
    a.H = H;
    a.restore = restore;
    if (!e->pool || i < 0 || i >= e->pfx.size() || slot >= e->kv_t.n_slots || h_row >= e->wt.max_rows) return -1;
    return launch_prefix_move(e->s, a);
}

// what is wrong with a rules block (q3e_admit_ruled's ranges), or null
static const char* rules_error(const q3e_slot_rules& r) {
    if (!(std::isfinite(r.rep_penalty) && r.rep_penalty >= 1.f)) return "rep_penalty must be finite and >= 1";
    if (r.rep_window < 0 || r.rep_window > 30) return "rep_window must be 0..30";
    if (!(std::isfinite(r.eos_boost) && r.eos_boost >= 0.f)) return "eos_boost must be finite and >= 0";
    if (!(std::isfinite(r.eos_force) && r.eos_force >= 0.f)) return "eos_force must be finite and >= 0";
    if (r.min_frames < 0) return "min_frames must be >= 0";
    if (!(r.cp_top_p > 0.f && r.cp_top_p <= 1.f)) return "cp_top_p must be in (0, 1]";
    if (r.reserved[0] || r.reserved[1]) return "reserved must be 0";
    return nullptr;
}

// q3e_admit (keys == NULL), q3e_admit_keyed (prompt_frames == NULL), q3e_admit_prompted (rules == NULL) and q3e_admit_ruled
static int admit_slots(Engine* e, int n, const int32_t* slots, const float* prefix, const int32_t* n_rows, const int32_t* n_text,
                       const q3e_slot_params* params, const uint64_t* keys, int32_t* hit, const int32_t* prompt_codes,
                       const int32_t* prompt_frames, const q3e_slot_rules* rules = nullptr) {
    if (!e || !e->slot_mode || n <= 0 || n > e->B || !slots || !prefix || !n_rows || !n_text || !params) {
        if (e && !e->slot_mode) Q3_LOG("q3e_admit: the batch was not opened with q3e_open");
        return -1;
    }
    if (rules && !e->rules) {
        Q3_LOG("q3e_admit_ruled: no sampler rules are reserved (q3e_rules_reserve)");
        return -1;
    }
    std::vector<SlotParams> sp(n);
    std::vector<SlotRules> kr(rules ? n : 0);        // the rules entries as the kernels read them
    std::vector<int32_t> n_prompt(n, 0), n_tot(n);   // prompt frames, and the rows the utterance's pass prefills
    size_t n_codes = 0;
    for (int u = 0; u < n; u++) {
        const q3e_slot_params& p = params[u];
        if (prompt_frames) n_prompt[u] = prompt_frames[u];
        if (n_prompt[u] < 0 || n_prompt[u] > e->prefill_rows || n_rows[u] <= 0 || (n_prompt[u] > 0 && !prompt_codes)) {
            Q3_LOG("q3e_admit: utterance %d: %d prefix rows, %d prompt frames", u, n_rows[u], n_prompt[u]);
            return -1;
        }
        n_tot[u] = n_rows[u] + n_prompt[u];
        if (!check_slot_list("q3e_admit", u, slots, e->B)) return -1;
        if (p.max_frames <= 0 || p.max_frames > e->max_frames) {
            Q3_LOG("q3e_admit: utterance %d: a budget of %d frames is outside 1..%d", u, p.max_frames, e->max_frames);
            return -1;
        }
        if (!check_fit(e, "q3e_admit", u, n_tot[u], p.max_frames)) return -1;
        for (size_t i = n_codes * 16; i < (n_codes + n_prompt[u]) * 16; i++) {
            // (column 0 is an audio id of the talker, the sampler's audio_vocab; the others index the code predictor's tables)
            const int32_t id = prompt_codes[i], vocab = e->m->cfg.cp_vocab;
            if (id < 0 || id >= vocab) {
                Q3_LOG("q3e_admit: utterance %d: prompt frame %zu holds id %d in column %zu (vocabulary %d)", u, i / 16 - n_codes,
                       id, i % 16, vocab);
                return -1;
            }
        }
        n_codes += n_prompt[u];
        if (!(std::isfinite(p.temperature) && p.temperature >= 0.f) || !(std::isfinite(p.cp_temperature) && p.cp_temperature >= 0.f) ||
            !(p.top_p > 0.f && p.top_p <= 1.f)) {
            Q3_LOG("q3e_admit: utterance %d: temperatures must be finite and >= 0, top_p in (0, 1]", u);
            return -1;
        }
        if (rules) {
            const q3e_slot_rules& q = rules[u];
            if (const char* why = rules_error(q)) {
                Q3_LOG("q3e_admit_ruled: utterance %d: %s", u, why);
                return -1;
            }
            kr[u].rep_penalty = q.rep_penalty;
            kr[u].rep_window = q.rep_window;
            kr[u].eos_boost = q.eos_boost;
            kr[u].eos_force = q.eos_force;
            // counted as the device counts: the prompt's frames are in n_past (saturating: the sum never wraps)
            kr[u].min_past = q.min_frames > INT32_MAX - n_prompt[u] ? INT32_MAX : n_prompt[u] + q.min_frames;
            kr[u].cp_top_p = q.cp_top_p;
        }
        sp[u].max_frames = n_prompt[u] + p.max_frames;   // the device counts the prompt's frames with the emitted ones (n_past)
        sp[u].t_temp = p.temperature;
        sp[u].t_top_k = p.top_k;
        sp[u].t_top_p = p.top_p;
        sp[u].c_temp = p.cp_temperature;
        sp[u].c_top_k = p.cp_top_k;
        sp[u].seed = mix_seed(p.seed, (unsigned long long)(uint32_t)p.utt + 1ull, 0x9E3779B97F4A7C15ull);   // mix(seed, utt)
        sp[u].no_row = 1;
        if ((p.reserved & 2) && !(p.reserved & 1)) {
            Q3_LOG("q3e_admit: utterance %d: bit 1 of reserved (text after a codec prompt) needs bit 0 (a text slot)", u);
            return -1;
        }
        if (p.reserved & 1) {
            if (!e->text) {
                Q3_LOG("q3e_admit: utterance %d is a text slot, but no text rows are reserved (q3e_text_reserve)", u);
                return -1;
            }
            if (n_prompt[u] && !(p.reserved & 2)) {
                Q3_LOG("q3e_admit: utterance %d: a text slot takes no codec prompt", u);
                return -1;
            }
            sp[u].flags = 3;   // a text slot; EOS masked until the final push
            // its rows are counted from the first generated frame: the sampler's hold test takes the prompt off n_past
            sp[u].prompt = n_prompt[u];
        }
    }
    Q3_HIP(hipStreamSynchronize(e->s), -1);
    std::vector<int32_t> hits(n, 0);
    const int rc = timed_prefill(e, [&]() -> int {
        for (int u = 0; u < n; u++) {   // (a text slot's n_text comes with its final push)
            if (reset_rows(e, slots[u], 1, RowStart::fresh, n_rows + u, sp[u].flags ? nullptr : n_text + u)) return -1;
            Q3_HIP(hipMemcpyAsync(e->d_slots + slots[u], &sp[u], sizeof(SlotParams), hipMemcpyHostToDevice, e->s), -1);
            // (reset_rows has written the defaults)
            if (rules) Q3_HIP(hipMemcpyAsync(e->rules->rules + slots[u], &kr[u], sizeof(SlotRules), hipMemcpyHostToDevice, e->s), -1);
        }
        Q3_HIP(hipStreamSynchronize(e->s), -1);
        // one prefill per utterance: the ragged prefill's tiles follow the rows of its pass, so sharing a pass with another
        // request's utterance would change this one's sums
        const int H = e->m->cfg.hidden;
        size_t row_off = 0, code_off = 0;
        for (int u = 0; u < n; row_off += n_rows[u], code_off += n_prompt[u], u++) {
            const int b = slots[u];
            const uint64_t k0 = keys ? keys[2 * u] : 0, k1 = keys ? keys[2 * u + 1] : 0;
            // a codec prompt's frames are rows of the utterance like the prefix's: one pass prefills them all, and an entry
            // of the cache holds them all.  The codes are read on a hit too: the ring is rebuilt from them.
            if (n_prompt[u])
                Q3_HIP(hipMemcpyAsync(e->d_prompt, prompt_codes + code_off * 16, sizeof(int32_t) * 16 * (size_t)n_prompt[u],
                                      hipMemcpyHostToDevice, e->s), -1);
            const PrefixIndex::Lookup l = e->pfx.lookup(k0, k1, n_tot[u]);
            if (l.what == PrefixIndex::HIT) {
                if (n_prompt[u] && prompt_launch(e, b, n_prompt[u], 0, false)) return -1;
                // the KV rows, and the last row's residual where a prefill of one utterance leaves it for the same final
                // norm launch (the residual stream is scratch between two frame steps, as it is for a prefill)
                if (prefix_move(e, l.entry, b, n_tot[u], 0, 1)) return -1;
                Q3_HIP(hipMemsetAsync(e->d_lastrow + b, 0, sizeof(int), e->s), -1);
                if (prefill_final_norm(e, b, 1, e->B)) return -1;
                e->pfx.hit(l);
                hits[u] = 1;
                continue;
            }
            if (prefill_ids(e, 1, &b, prefix + row_off * H, &n_tot[u], e->B, n_prompt[u])) return -1;
            const int at = e->pfx.miss(l);   // keyed, and it fits the pool: the entry to keep it in
            if (at < 0) continue;
            if (prefix_move(e, at, b, n_tot[u], n_tot[u] - 1, 0)) return -1;
            e->pfx.store(at, k0, k1, n_tot[u]);
        }
        return head_all_rows(e);
    });
    if (rc) return -1;
    for (int u = 0; u < n; u++) {
        e->book.admit(slots[u], params[u].max_frames, sp[u].flags != 0, n_prompt[u]);
        e->h_sp[slots[u]] = sp[u];
    }
    if (hit) memcpy(hit, hits.data(), sizeof(int32_t) * n);
    return 0;
}

int q3e_admit(void* ee, int n, const int32_t* slots, const float* prefix, const int32_t* n_rows, const int32_t* n_text,
              const q3e_slot_params* params) {
    return admit_slots((Engine*)ee, n, slots, prefix, n_rows, n_text, params, nullptr, nullptr, nullptr, nullptr);
}

int q3e_admit_keyed(void* ee, int n, const int32_t* slots, const float* prefix, const int32_t* n_rows, const int32_t* n_text,
                    const q3e_slot_params* params, const uint64_t* keys, int32_t* hit) {
    return admit_slots((Engine*)ee, n, slots, prefix, n_rows, n_text, params, keys, hit, nullptr, nullptr);
}

int q3e_admit_prompted(void* ee, int n, const int32_t* slots, const float* prefix, const int32_t* n_rows, const int32_t* n_text,
                       const q3e_slot_params* params, const uint64_t* keys, int32_t* hit, const int32_t* prompt_codes,
                       const int32_t* prompt_frames) {
    return admit_slots((Engine*)ee, n, slots, prefix, n_rows, n_text, params, keys, hit, prompt_codes, prompt_frames);
}

int q3e_admit_ruled(void* ee, int n, const int32_t* slots, const float* prefix, const int32_t* n_rows, const int32_t* n_text,
                    const q3e_slot_params* params, const uint64_t* keys, int32_t* hit, const int32_t* prompt_codes,
                    const int32_t* prompt_frames, const q3e_slot_rules* rules) {
    return admit_slots((Engine*)ee, n, slots, prefix, n_rows, n_text, params, keys, hit, prompt_codes, prompt_frames, rules);
}

void q3e_default_rules(q3e_slot_rules* out) {
    if (!out) return;
    const SlotRules d;   // the constants of llamacpp_talker_server.py:163-206
    out->rep_penalty = d.rep_penalty;
    out->rep_window = d.rep_window;
    out->eos_boost = d.eos_boost;
    out->eos_force = d.eos_force;
    out->min_frames = 0;
    out->cp_top_p = d.cp_top_p;
    out->reserved[0] = out->reserved[1] = 0;
}

int q3e_rules_reserve(void* ee, int on) {
    Engine* e = (Engine*)ee;
    if (!e) return -1;
    if (e->slot_mode) {
        Q3_LOG("q3e_rules_reserve: a per-slot batch is open (call before q3e_open)");
        return -1;
    }
    Q3_HIP(hipStreamSynchronize(e->s), -1);
    if ((on != 0) == (e->rules != nullptr)) return 0;
    e->rules.reset();
    if (!on) return 0;
    auto r = std::make_unique<RuleSets>();
    r->seen_words = (e->m->cfg.cp_vocab + 31) / 32;
    r->defaults.assign(e->max_batch, SlotRules());
    if (!r->mem.alloc(&r->rules, sizeof(SlotRules) * e->max_batch) ||
        !r->mem.alloc_zeroed(&r->seen, sizeof(unsigned) * (size_t)e->max_batch * r->seen_words, e->s)) {
        Q3_LOG("q3e_rules_reserve: allocation failed");
        return -1;
    }
    Q3_HIP(hipMemcpyAsync(r->rules, r->defaults.data(), sizeof(SlotRules) * e->max_batch, hipMemcpyHostToDevice, e->s), -1);
    Q3_HIP(hipStreamSynchronize(e->s), -1);
    e->rules = std::move(r);
    return 0;
}

int q3e_prefix_cache(void* ee, int n_entries, int max_rows) {
    Engine* e = (Engine*)ee;
    if (!e || n_entries < 0 || max_rows < 0 || (n_entries > 0 && max_rows == 0)) {
        if (e) Q3_LOG("q3e_prefix_cache: %d entries of %d rows", n_entries, max_rows);
        return -1;
    }
    if (max_rows > e->n_ctx) max_rows = e->n_ctx;   // a longer prefix fits no slot
    if (n_entries == 0) max_rows = 0;
    Q3_HIP(hipStreamSynchronize(e->s), -1);
    std::unique_ptr<PrefixPool> pool;
    if (n_entries > 0) {
        pool = std::make_unique<PrefixPool>();
        const int H = e->m->cfg.hidden;
        const size_t elems = (size_t)e->kv_t.n_layers * 2 * e->kv_t.n_kv * max_rows * 128;
        if (!pool->mem.alloc(&pool->kv, sizeof(half_t) * elems * n_entries) ||
            !pool->mem.alloc(&pool->state, sizeof(float) * (size_t)(H + H / 16) * n_entries)) {
            Q3_LOG("q3e_prefix_cache: allocation of %zu bytes failed", sizeof(half_t) * elems * n_entries);
            return -1;   // the pool that was there stays
        }
    }
    e->pool = std::move(pool);
    e->pfx.resize(n_entries, max_rows);
    return 0;
}

int q3e_prefix_stats(void* ee, int64_t* out) {
    Engine* e = (Engine*)ee;
    if (!e || !out) return -1;
    const PrefixIndex& p = e->pfx;
    const int64_t stats[6] = {p.hits, p.misses, p.stores, p.evictions, p.too_long, p.used()};
    memcpy(out, stats, sizeof(stats));
    return 0;
}

int q3e_text_reserve(void* ee, int max_rows) {
    Engine* e = (Engine*)ee;
    if (!e || max_rows < 0 || max_rows > e->max_frames) {
        if (e) Q3_LOG("q3e_text_reserve: %d rows are outside 0..max_frames=%d", max_rows, e->max_frames);
        return -1;
    }
    const int busy = e->slot_mode ? e->book.first_live_text() : -1;
    if (busy >= 0) {
        Q3_LOG("q3e_text_reserve: slot %d holds a live text utterance", busy);
        return -1;
    }
    Q3_HIP(hipStreamSynchronize(e->s), -1);
    if (max_rows == (e->text ? e->text->cap : 0)) return 0;
    auto t = std::make_unique<TextRows>();
    t->cap = max_rows;
    t->hold = e->hold();   // a new size keeps the mode; with no rows left there is nothing to hold a slot for
    e->text.reset();
    if (max_rows == 0) return 0;
    const size_t n = (size_t)e->max_batch * max_rows * e->m->cfg.hidden;
    if (!t->mem.alloc_zeroed(&t->rows, sizeof(float) * n, e->s) || !t->mem.alloc_zeroed(&t->avail, sizeof(int) * e->max_batch, e->s) ||
        !t->mem.alloc_zeroed(&t->held, sizeof(int) * e->max_batch, e->s)) {
        Q3_LOG("q3e_text_reserve: allocation of %zu bytes failed", sizeof(float) * n);
        return -1;
    }
    Q3_HIP(hipStreamSynchronize(e->s), -1);
    e->text = std::move(t);
    return 0;
}

int q3e_push_text(void* ee, int slot, const float* rows, int n, int final, int n_text_total) {
    Engine* e = (Engine*)ee;
    if (!e || !e->slot_mode || !e->text || slot < 0 || slot >= e->B || n < 0 || (n > 0 && !rows)) return -1;
    const int have = e->book[slot].text_rows;
    if (!e->book.live_text(slot)) {
        Q3_LOG("q3e_push_text: slot %d holds no live text utterance", slot);
        return -1;
    }
    if (e->book[slot].text_final) {
        Q3_LOG("q3e_push_text: the text of slot %d has ended", slot);
        return -1;
    }
    if (have + n > e->text->cap) {
        Q3_LOG("q3e_push_text: slot %d: %d + %d rows exceed the reservation of %d", slot, have, n, e->text->cap);
        return -1;
    }
    if (final && n_text_total < 0) return -1;
    const int H = e->m->cfg.hidden;
    for (size_t i = 0; i < (size_t)n * H; i++)
        if (!std::isfinite(rows[i])) {
            Q3_LOG("q3e_push_text: slot %d: row %d holds a non-finite value", slot, (int)(i / H));
            return -1;
        }
    // the rows first, then the counter that makes them visible; q3e_run has synchronised, so no frame is in flight
    if (n > 0)
        Q3_HIP(hipMemcpyAsync(e->text->rows + ((size_t)slot * e->text->cap + have) * H, rows, sizeof(float) * (size_t)n * H,
                              hipMemcpyHostToDevice, e->s), -1);
    e->up_i[0] = have + n;
    Q3_HIP(hipMemcpyAsync(e->text->avail + slot, &e->up_i[0], sizeof(int), hipMemcpyHostToDevice, e->s), -1);
    SlotParams sp = e->h_sp[slot];
    if (final) {   // the reference's EOS rules from the next sampled frame on: mask lifted, n_text known
        sp.flags = 1;
        e->up_i[1] = n_text_total;
        Q3_HIP(hipMemcpyAsync(e->d_slots + slot, &sp, sizeof(SlotParams), hipMemcpyHostToDevice, e->s), -1);
        Q3_HIP(hipMemcpyAsync(e->d_ntext + slot, &e->up_i[1], sizeof(int), hipMemcpyHostToDevice, e->s), -1);
    }
    Q3_HIP(hipStreamSynchronize(e->s), -1);   // the caller's rows (and the locals) are their own again on return
    e->book.push(slot, n, final != 0);
    if (final) e->h_sp[slot] = sp;
    return 0;
}

int q3e_text_state(void* ee, int32_t* rows, int32_t* starved) {
    Engine* e = (Engine*)ee;
    if (!e || !e->slot_mode || e->B <= 0) return -1;
    for (int b = 0; b < e->B; b++) {
        if (rows) rows[b] = e->book[b].text_rows;   // (only a text slot is pushed rows)
        if (starved) starved[b] = e->book.starved(b);
    }
    return 0;
}

int q3e_text_hold(void* ee, int on) {
    Engine* e = (Engine*)ee;
    if (!e) return -1;
    if (!e->text) {
        Q3_LOG("q3e_text_hold: no text rows are reserved (q3e_text_reserve)");
        return -1;
    }
    if (e->slot_mode) {
        Q3_LOG("q3e_text_hold: a per-slot batch is open (call between q3e_text_reserve and q3e_open)");
        return -1;
    }
    e->text->hold = on != 0;
    return 0;
}

int q3e_text_held(void* ee, int64_t* held_steps) {
    Engine* e = (Engine*)ee;
    if (!e || !e->slot_mode || e->B <= 0 || !held_steps) return -1;
    for (int b = 0; b < e->B; b++) held_steps[b] = e->book[b].held;
    return 0;
}

int q3e_release(void* ee, int n, const int32_t* slots) {
    Engine* e = (Engine*)ee;
    if (!e || !e->slot_mode || n < 0 || (n > 0 && !slots)) return -1;
    for (int u = 0; u < n; u++)
        if (slots[u] < 0 || slots[u] >= e->B) {
            Q3_LOG("q3e_release: slot %d is out of range (batch of %d)", slots[u], e->B);
            return -1;
        }
    for (int u = 0; u < n; u++) {
        Q3_HIP(hipMemsetD32Async((hipDeviceptr_t)(e->d_done + slots[u]), 1, 1, e->s), -1);
        e->book.release(slots[u]);
    }
    Q3_HIP(hipStreamSynchronize(e->s), -1);
    return 0;
}

int q3e_get_hidden(void* ee, float* out) {
    Engine* e = (Engine*)ee;
    if (!e || !out || e->B <= 0) return -1;
    Q3_HIP(hipMemcpyAsync(out, e->wt.hidden_f32, sizeof(float) * (size_t)e->B * e->m->cfg.hidden, hipMemcpyDeviceToHost, e->s), -1);
    Q3_HIP(hipStreamSynchronize(e->s), -1);
    return 0;
}

double q3e_step_weight_bytes(void* ee) {
    Engine* e = (Engine*)ee;
    if (!e) return 0.0;
    const ModelCfg& c = e->m->cfg;
    const double head = 2.0 * c.hidden;
    double bytes = (double)e->m->talker.weight_bytes + head * c.talker_vocab +
                   (double)(c.cp_groups + 1) * (double)e->m->cp.weight_bytes + head * c.cp_vocab * c.cp_groups;
    int row0 = 0, R = e->B;
    if (e->B > 0) chain_rows(e, 0, row0, R);
    if (R > 0 && e->m->cp_qkv_serves(R)) {
        // positions 2.. of the code predictor take layer 0's q|k|v from the table: one f32 row per utterance instead of the weights
        const double qkv_ld = (double)(c.n_heads + 2 * c.n_kv) * c.head_dim;
        bytes -= (double)(c.cp_groups - 1) * (qkv_ld * c.hidden * 2.0 - 4.0 * qkv_ld * e->B);
    }
    return bytes;
}

}  // extern "C"
