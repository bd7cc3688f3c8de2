// q3_sample.hip -- gfx950 (MI355X, CDNA4) samplers of the Qwen3-TTS frame loop.  Wave = 64 lanes.
//
// Hot-path map (reference file:line each kernel stands in for):
//   talker_sample   llamacpp_talker_server.py:163-206 (greedy form) on device.
//   cp_argmax       code_predictor_server.py:87-92,128-137 (greedy) + next
//                   embedding gather, and tts_client.py:199-208 feedback sum.
#include "q3_kdev.h"

namespace q3 {

// ---------------------------------------------------------------------------
// talker sampling, greedy form of llamacpp_talker_server.py:163-206
// ---------------------------------------------------------------------------
__device__ __forceinline__ void block_argmax(float& v, int& idx, float* sv, int* si) {
    // lowest index wins ties
    group_argmax_down<64>(v, idx);
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sv[w] = v;
        si[w] = idx;
    }
    __syncthreads();
    v = sv[0];
    idx = si[0];
    for (int i = 1; i < nw; i++)
        if (sv[i] > v || (sv[i] == v && si[i] < idx)) {
            v = sv[i];
            idx = si[i];
        }
    __syncthreads();
}

// ---- stochastic sampling on the device (top-k / temperature / optional top-p) -----------------
// Counter-based generator: the draw depends only on (seed, row, frame, group), so a captured graph
// replays deterministically for a given seed.
__device__ __forceinline__ float uniform01(unsigned long long seed, unsigned row, unsigned frame, unsigned group) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (1ull + row + ((unsigned long long)frame << 20) +
                                                            ((unsigned long long)group << 44));
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (float)(z >> 40) * (1.0f / 16777216.0f);   // 24 bits -> [0, 1)
}

// NaN logits: numpy's argmax (the reference's greedy limit) lets the first NaN win; the device does the same by
// ordering a NaN as +inf.  A row whose best key is not finite (NaN, +inf, or nothing but -inf) has no softmax:
// the sampler then returns that best index instead of drawing (the reference would raise inside np.random.choice
// and answer -2; a device kernel cannot raise, and must never index with an invalid winner).
__device__ __forceinline__ float nan_as_inf(float l) { return l != l ? INFINITY : l; }

constexpr int SAMPLE_SEL_CAP = 64;      // top_k up to this: k selection rounds; beyond (or "all"): a full LDS sort
constexpr int SAMPLE_SORT_CAP = 4096;   // largest vocabulary the full sort handles (talker 3072, code predictor 2048)
// top_k as the reference means it: <= 0 or >= n keeps every entry (np.argpartition is skipped there)
__host__ __device__ __forceinline__ int effective_top_k(int top_k, int n) { return (top_k <= 0 || top_k > n) ? n : top_k; }
__host__ __device__ __forceinline__ int sample_sort_len(int n) {
    int p = 64;
    while (p < n) p <<= 1;
    return p;
}
// dynamic LDS bytes the samplers need for a vocabulary of n at this top_k (0 when greedy)
static size_t sample_lds_bytes(int n, int top_k, float temperature) {
    if (!(temperature > 1e-6f)) return 0;
    return effective_top_k(top_k, n) <= SAMPLE_SEL_CAP ? (size_t)n * 4 : (size_t)sample_sort_len(n) * 8;
}

// lg: n processed logits in LDS (destroyed; capacity n floats, or sample_sort_len(n) floats followed by as many
// ints when top_k needs the full sort).  Keeps the top_k largest (ties: lowest index first), applies
// softmax((l - max) / max(T, 1e-6)) like the reference samplers, optionally keeps the smallest prefix of the
// descending order whose mass reaches top_p (llamacpp_talker_server.py:199-205), and draws with u.
// All threads of the block must call it; every thread returns the chosen index (always in [0, n)).
__device__ int block_sample_topk(float* lg, int n, int top_k, float temperature, float top_p, float u, float* sv,
                                 int* si, float* selv, int* seli) {
    __shared__ int chosen;
    top_k = effective_top_k(top_k, n);
    const float inv_t = 1.0f / fmaxf(temperature, 1e-6f);
    if (top_k <= SAMPLE_SEL_CAP) {
        int found = 0;
        for (int k = 0; k < top_k; k++) {
            float best = -INFINITY;
            int bidx = 0x7fffffff;
            for (int v = threadIdx.x; v < n; v += blockDim.x) {
                const float l = lg[v];
                if (l > best) {
                    best = l;
                    bidx = v;
                }
            }
            block_argmax(best, bidx, sv, si);
            if (bidx >= n) break;            // nothing above -inf is left (block-uniform)
            if (threadIdx.x == 0) {
                selv[k] = best;
                seli[k] = bidx;
                lg[bidx] = -INFINITY;
            }
            found = k + 1;
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            int pick = 0;
            if (found > 0 && !(selv[0] < INFINITY)) pick = seli[0];       // NaN / +inf on top: no softmax exists
            else if (found > 0) {
                // the selection is in descending order: selv[0] is the maximum (held in a register: the loop overwrites
                // selv[0] with its weight, 1, in its first round)
                const float top = selv[0];
                float sum = 0.f;
                for (int k = 0; k < found; k++) {
                    selv[k] = expf((selv[k] - top) * inv_t);
                    sum += selv[k];
                }
                int keep = found;
                if (top_p > 0.f && top_p < 1.f) {
                    float c = 0.f;
                    for (int k = 0; k < found; k++) {
                        c += selv[k] / sum;
                        if (c >= top_p) {   // np.searchsorted(cumsum, top_p) + 1 entries
                            keep = k + 1;
                            break;
                        }
                    }
                    sum = 0.f;
                    for (int k = 0; k < keep; k++) sum += selv[k];
                }
                float c = 0.f;
                pick = seli[keep - 1];
                const float target = u * sum;
                for (int k = 0; k < keep; k++) {
                    c += selv[k];
                    if (target < c) {
                        pick = seli[k];
                        break;
                    }
                }
            }
            chosen = pick;
        }
        __syncthreads();
        return chosen;
    }
    // ---- top_k beyond the selection cap (or "all"): bitonic sort of (key, index), descending key, ascending index ----
    const int n2 = sample_sort_len(n);
    int* li = (int*)(lg + n2);
    for (int v = threadIdx.x; v < n2; v += blockDim.x) {
        if (v >= n) lg[v] = -INFINITY;
        li[v] = v;
    }
    __syncthreads();
    for (int k2 = 2; k2 <= n2; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n2; i += blockDim.x) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const float a0 = lg[i], a1 = lg[ixj];
                    const int i0 = li[i], i1 = li[ixj];
                    const bool before = a0 > a1 || (a0 == a1 && i0 < i1);   // element i belongs ahead of element ixj
                    const bool desc = (i & k2) == 0;
                    if (desc ? !before : before) {
                        lg[i] = a1;
                        lg[ixj] = a0;
                        li[i] = i1;
                        li[ixj] = i0;
                    }
                }
            }
            __syncthreads();
        }
    if (threadIdx.x == 0) {
        int pick = li[0] < n ? li[0] : 0;
        const float top = lg[0];
        if (top < INFINITY && top > -INFINITY) {
            float sum = 0.f;
            int found = 0;
            for (int k = 0; k < top_k; k++) {
                if (!(lg[k] > -INFINITY)) break;
                lg[k] = expf((lg[k] - top) * inv_t);
                sum += lg[k];
                found = k + 1;
            }
            int keep = found;
            if (top_p > 0.f && top_p < 1.f) {
                float c = 0.f;
                for (int k = 0; k < found; k++) {
                    c += lg[k] / sum;
                    if (c >= top_p) {
                        keep = k + 1;
                        break;
                    }
                }
                sum = 0.f;
                for (int k = 0; k < keep; k++) sum += lg[k];
            }
            float c = 0.f;
            pick = li[keep - 1];
            const float target = u * sum;
            for (int k = 0; k < keep; k++) {
                c += lg[k];
                if (target < c) {
                    pick = li[k];
                    break;
                }
            }
        }
        chosen = pick;
    }
    __syncthreads();
    return chosen;
}

// The row's entry of a per-slot array the host writes before the launch: scalar loads, see uniform_load.
template <class T>
__device__ __forceinline__ T uniform_entry(const T* p, int r) {
    static_assert(sizeof(T) % 4 == 0, "the entry is read as words");
    constexpr int NW = (int)(sizeof(T) / 4);
    const __attribute__((address_space(4))) int* q = (const __attribute__((address_space(4))) int*)(p + r);
    int w[NW];
#pragma unroll
    for (int i = 0; i < NW; i++) w[i] = q[i];
    T e;
    __builtin_memcpy(&e, w, sizeof(e));
    return e;
}
// the per-slot parameter array (q3e_admit) and the per-slot rules array (q3e_admit_ruled)
__device__ __forceinline__ SlotParams uniform_slot(const SlotParams* p, int r) { return uniform_entry(p, r); }
__device__ __forceinline__ SlotRules uniform_rules(const SlotRules* p, int r) { return uniform_entry(p, r); }

// SLOTS: per-slot mode -- budget, temperature, top-k, top-p and draw key of the row come from a.slots[r]
// RULES (with SLOTS): a.rules[r] / a.seen[r] where given (TalkerSampleArgs); a kernel of its own, so that a launch without
// them runs the code it always did
// SCORES: a.scores gets the log-probability of the id the stream continues with (TalkerSampleArgs::scores); kernels of their
// own again.  Every thread carries an online (max, sum of exp) pair of the RAW allowed logits through the loop that reads
// them; the pairs meet in the wave (wave_max, wave_sum), then in LDS in wave order, so the value has one summation order
// and is the same bits run to run.  The barriers of the winner's reduction order the LDS words: no barrier is added.
template <bool SLOTS, bool RULES = false, bool SCORES = false>
__device__ __forceinline__ void talker_sample_row(const TalkerSampleArgs& a) {
    Q3_TL(42);
    __shared__ float sv[16];
    __shared__ int si[16];
    __shared__ float sc_wm[SCORES ? 16 : 1], sc_ws[SCORES ? 16 : 1];   // per wave: maximum, sum of exp(z - maximum)
    float sc_m = -INFINITY, sc_s = 0.f;
    __shared__ int win[32];
    __shared__ int nwin;
    const int r = a.row0 + blockIdx.x;
    const int RT = a.R_total > 0 ? a.R_total : a.R;
    const int np = uniform_load(a.n_past + r);
    const int nt = uniform_load(a.n_text + r);
    const bool was_done = uniform_load(a.done + r) != 0;
    float temperature = a.temperature, top_p = a.top_p;
    int top_k = a.top_k, max_frames = a.max_frames;
    int slot_flags = 0;   // SLOTS only (bit 1: the row's EOS is masked -- a text slot before its final push)
    if constexpr (SLOTS) {
        const SlotParams sp = uniform_slot(a.slots, r);
        temperature = sp.t_temp;
        top_p = sp.t_top_p;
        top_k = sp.t_top_k;
        max_frames = sp.max_frames;
        slot_flags = sp.flags;
        if (a.text_avail) {
            // held text slots (q3e_text_hold): the row's next frame has no text row yet.  Scalar values only, so the
            // whole workgroup leaves together, before the first barrier and before it has read a logit.  Rows are counted
            // by the frames the slot generated: a codec prompt's frames (sp.prompt of n_past) need no row.
            const int avail = uniform_load(a.text_avail + r);
            const int gen = np - sp.prompt;
            const bool held = (slot_flags & 3) == 3 && !was_done && gen >= 1 && gen >= avail && np < max_frames;
            if (threadIdx.x == 0) a.held[r] = held ? 1 : 0;
            if (held) return;
        }
    }
    // the rules of the row: the launch's constants, or the row's entry of a.rules (all uniform)
    float rep_penalty = a.rep_penalty;
    int rep_window = 30;
    double eos_boost = 15.0, eos_force = 2.0;
    bool add_boost = true, may_force = true, eos_early = false;   // eos_early: n_past < min_past, EOS cannot be chosen yet
    const unsigned* seen_row = nullptr;   // rep_window 0: the repetition test reads the row's seen-set, not the ring
    if constexpr (RULES) {
        if (a.rules) {
            const SlotRules ru = uniform_rules(a.rules, r);
            rep_penalty = ru.rep_penalty;
            rep_window = ru.rep_window < 0 ? 0 : ru.rep_window > 30 ? 30 : ru.rep_window;   // (win holds 32)
            eos_boost = (double)ru.eos_boost;
            eos_force = (double)ru.eos_force;
            add_boost = ru.eos_boost != 0.f;
            may_force = ru.eos_force != 0.f;
            eos_early = np < ru.min_past;
            if (rep_window == 0) seen_row = a.seen + (size_t)r * ((a.audio_vocab + 31) / 32);
        }
    }
    if (threadIdx.x == 0) nwin = np < rep_window ? np : rep_window;
    if (threadIdx.x < rep_window && threadIdx.x < np) {
        // last 30 (rep_window) emitted tokens (ring of 32)
        win[threadIdx.x] = a.past[r * 32 + ((np - 1 - threadIdx.x) & 31)];
    }
    __syncthreads();
    // adaptive EOS boost (python floats = doubles; numpy>=2 adds it as a float32)
    double progress = 0.0;
    float boost = 0.f;
    bool force_eos = false;
    if (nt > 0) {
        const double expected = (double)nt * 3.0;
        progress = (double)np / expected;
        if (progress > 0.8) {
            double b = (progress - 0.8) / 0.7;
            if (b > 1.0) b = 1.0;
            boost = (float)(b * eos_boost);
        }
        if (may_force && progress > eos_force) force_eos = true;
    }
    const bool eos_masked = a.ignore_eos || (SLOTS && (slot_flags & 2)) || (RULES && eos_early);
    float best = -INFINITY;
    int bidx = 0x7fffffff;
    const int nw_ = nwin;
    extern __shared__ float slg[];   // [V] processed logits, only when sampling stochastically
    __shared__ float selv[64];
    __shared__ int seli[64];
    const bool stochastic = temperature > 1e-6f;
    for (int v = threadIdx.x; v < a.V; v += blockDim.x) {
        float l = nan_as_inf(a.logits[(size_t)r * a.V + v]);
        if constexpr (SCORES) {
            // (a -inf entry adds exp(-inf) = 0 whatever the maximum: skipping it keeps -inf - -inf out of the pair)
            if ((v < a.audio_vocab || v == a.eos) && l > -INFINITY) {
                if (l > sc_m) {
                    sc_s = sc_s * expf(sc_m - l) + 1.f;
                    sc_m = l;
                } else {
                    sc_s += expf(l - sc_m);
                }
            }
        }
        if (v >= a.audio_vocab && v != a.eos) l = -1e10f;
        if (v == a.eos) {
            if (eos_masked) l = -1e10f;
            else if (nt > 0 && progress > 0.8 && add_boost) l += boost;
        }
        bool rep = false;
        for (int i = 0; i < nw_; i++) rep |= (win[i] == v);
        if constexpr (RULES)   // (written by earlier launches of this kernel: a vector load, not a scalar one)
            if (seen_row && v < a.audio_vocab) rep = (seen_row[v >> 5] >> (v & 31)) & 1u;
        if (rep) l = l > 0.f ? __fdiv_rn(l, rep_penalty) : l * rep_penalty;
        if (stochastic) slg[v] = l;
        if (l > best || (l == best && v < bidx)) {
            best = l;
            bidx = v;
        }
    }
    if constexpr (SCORES) {
        const float wm = wave_max(sc_m);
        const float ws = wave_sum(sc_m > -INFINITY ? sc_s * expf(sc_m - wm) : 0.f);
        if ((threadIdx.x & 63) == 0) {
            sc_wm[threadIdx.x >> 6] = wm;
            sc_ws[threadIdx.x >> 6] = ws;
        }
    }
    if (stochastic) {
        __syncthreads();
        float u;
        if constexpr (SLOTS) {
            const SlotParams sp = uniform_slot(a.slots, r);
            u = uniform01(sp.seed, sp.no_row ? 0u : (unsigned)r, (unsigned)a.n_frames[r], 0u);
        } else {
            u = uniform01(a.seed_ptr ? a.seed_ptr[r] : a.seed, (unsigned)r, (unsigned)a.n_frames[r], 0u);
        }
        bidx = block_sample_topk(slg, a.V, top_k, temperature, top_p, u, sv, si, selv, seli);
    } else {
        block_argmax(best, bidx, sv, si);
        if (bidx >= a.V) bidx = a.eos;   // unreachable (the mask leaves finite entries); never index with an invalid winner
    }
    if (threadIdx.x == 0) {
        int code = bidx;
        if (force_eos && !eos_masked) code = a.eos;
        bool fin = was_done || code == a.eos || code >= a.audio_vocab || (max_frames > 0 && np >= max_frames);
        const int f = a.n_frames[r];
        // per-slot batches live as long as the server: an ended row's counter stops one past the codes array (frame_cap + 1,
        // so the code predictor's frame f - 1 is past it too) instead of counting every step of the server's life
        if (!SLOTS || !fin || f <= a.frame_cap) a.n_frames[r] = f + 1;
        const bool keep = f < a.frame_cap;     // a frame beyond the codes array is not recorded (q3e_run never asks for one)
        int* fc = a.codes + ((size_t)(keep ? f : 0) * RT + r) * 16;
        // teacher forcing (tests): the decision is recorded, the forced id is what the stream continues with
        int used = code;
        if (a.forced && keep && !fin) {
            const int fz = a.forced[((size_t)f * RT + r) * 16];
            if (fz >= 0) used = fz;
        }
        if (fin || !keep) {
            a.done[r] = 1;
            if (keep) fc[0] = -1;
        } else {
            fc[0] = code;
            if constexpr (SCORES) {
                if (a.scores) {
                    const int nw = blockDim.x >> 6;
                    float m = sc_wm[0], sum = 0.f;
                    for (int i = 1; i < nw; i++) m = fmaxf(m, sc_wm[i]);
                    for (int i = 0; i < nw; i++) sum += sc_wm[i] > -INFINITY ? sc_ws[i] * expf(sc_wm[i] - m) : 0.f;
                    float zu = -INFINITY;   // an id outside the allowed set
                    if (used >= 0 && used < a.V && (used < a.audio_vocab || used == a.eos))
                        zu = nan_as_inf(a.logits[(size_t)r * a.V + used]);
                    // m = +inf, or nothing above -inf: the formula's own inf - inf
                    a.scores[((size_t)f * RT + r) * 16] = (m < INFINITY && m > -INFINITY) ? zu - m - logf(sum) : __builtin_nanf("");
                }
            }
            a.past[r * 32 + (np & 31)] = used;
            if constexpr (RULES)   // one workgroup owns the row: a plain read-modify-write (every read of the loop above is
                                   // behind the barriers of the winner's reduction)
                if (a.seen && used >= 0 && used < a.audio_vocab)
                    a.seen[(size_t)r * ((a.audio_vocab + 31) / 32) + (used >> 5)] |= 1u << (used & 31);
            a.n_past[r] = np + 1;
            a.pos[r] = a.pos0[r] + np;
        }
    }
}
__global__ void talker_sample_kernel(TalkerSampleArgs a) { talker_sample_row<false>(a); }
__global__ void talker_sample_kernel_slots(TalkerSampleArgs a) { talker_sample_row<true>(a); }
__global__ void talker_sample_kernel_rules(TalkerSampleArgs a) { talker_sample_row<true, true>(a); }
__global__ void talker_sample_kernel_scores(TalkerSampleArgs a) { talker_sample_row<false, false, true>(a); }
__global__ void talker_sample_kernel_slots_scores(TalkerSampleArgs a) { talker_sample_row<true, false, true>(a); }
__global__ void talker_sample_kernel_rules_scores(TalkerSampleArgs a) { talker_sample_row<true, true, true>(a); }

// per-slot mode: any row may take the sort path, so its LDS is reserved whatever the rows ask for (admitting a request
// never changes the captured launch)
static size_t sample_lds_bytes_slots(int n) { return (size_t)sample_sort_len(n) * 8; }

// what both samplers refuse: a vocabulary the LDS sort cannot hold, where a row may (per-slot mode) or will take it
static int sample_vocab_refused(const char* who, bool slots, int V, float temperature, int top_k) {
    if (slots && V > SAMPLE_SORT_CAP) {
        Q3_LOG("%s: a vocabulary of %d is beyond the per-slot sampler (sort cap %d)", who, V, SAMPLE_SORT_CAP);
        return -1;
    }
    if (temperature > 1e-6f && effective_top_k(top_k, V) > SAMPLE_SEL_CAP && V > SAMPLE_SORT_CAP) {
        Q3_LOG("%s: top_k=%d over a vocabulary of %d is beyond the device sampler (sort cap %d)", who, top_k, V, SAMPLE_SORT_CAP);
        return -1;
    }
    return 0;
}

int launch_talker_sample(hipStream_t s, const TalkerSampleArgs& a) {
    if (a.R <= 0) return 0;
    // held text slots are a per-slot feature: the kernel writes held[r] wherever text_avail is given
    if ((a.text_avail && !a.held) || ((a.text_avail || a.held) && !a.slots)) {
        Q3_LOG("talker_sample: text_avail / held need each other and per-slot mode (text_avail %p, held %p, slots %p)",
               (const void*)a.text_avail, (const void*)a.held, (const void*)a.slots);
        return -1;
    }
    // sampler rules are a per-slot feature too; a window of 0 reads the seen-set, so rules come with one
    if ((a.rules || a.seen) && (!a.slots || (a.rules && !a.seen) || a.audio_vocab <= 0)) {
        Q3_LOG("talker_sample: rules need seen, and both per-slot mode (rules %p, seen %p, slots %p)", (const void*)a.rules,
               (const void*)a.seen, (const void*)a.slots);
        return -1;
    }
    if (sample_vocab_refused("talker_sample", a.slots != nullptr, a.V, a.temperature, a.top_k)) return -1;
    const size_t lds = a.slots ? sample_lds_bytes_slots(a.V) : sample_lds_bytes(a.V, a.top_k, a.temperature);
    TalkerSampleArgs a2 = a;
    a2.tl_node = tl_next_node();
    // [scores][plain | slots | rules] (q3e_scores_reserve: the same choice among the kernels that also score)
    static void (*const kernels[2][3])(TalkerSampleArgs) = {
        {talker_sample_kernel, talker_sample_kernel_slots, talker_sample_kernel_rules},
        {talker_sample_kernel_scores, talker_sample_kernel_slots_scores, talker_sample_kernel_rules_scores}};
    hipLaunchKernelGGL(kernels[a.scores ? 1 : 0][(a.rules || a.seen) ? 2 : a.slots ? 1 : 0], dim3(a.R), dim3(256), lds, s, a2);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

// ---------------------------------------------------------------------------
// code-predictor argmax + gather / feedback
// ---------------------------------------------------------------------------
// One workgroup per row: the 2048 logits arrive as two float4 per thread (one round trip), one barrier
// picks the winner, then the next embedding row is gathered (second round trip).
// RULES (with SLOTS): a.rules[r].cp_top_p cuts the stochastic draw; a kernel of its own, as for the talker
// SCORES: a.scores gets the log-softmax of the id the stream continues with (CpArgmaxArgs::scores); kernels of their own.
// The block arg-max over the raw logits is the maximum; the sum of exp(z - max) comes from the registers that hold the
// logits, through one more block reduction (wave_sum, four LDS words added in wave order, one barrier).
template <bool SLOTS, bool RULES = false, bool SCORES = false>
__device__ __forceinline__ void cp_argmax_row(const CpArgmaxArgs& a) {
    if constexpr (SLOTS)
        Q3_FETCH_ARGS("s"(a.logits), "s"(a.V), "s"(a.H), "s"(a.row0), "s"(a.R_total), "s"(a.R), "s"(a.group), "s"(a.codes), "s"(a.n_frames),
                      "s"(a.frame_cap), "s"(a.next_table), "s"(a.h_out), "s"(a.ssq_out), "s"(a.xh_out), "s"(a.gamma_next),
                      "s"(a.talker_emb), "s"(a.slots), "s"(a.forced), "s"(a.next_qkv), "s"(a.qkv_out), "s"(a.qkv_ld),
                      "s"(a.text_rows), "s"(a.text_avail), "s"(a.text_cap), "s"(a.held));
    else
        Q3_FETCH_ARGS("s"(a.logits), "s"(a.V), "s"(a.H), "s"(a.row0), "s"(a.R_total), "s"(a.R), "s"(a.group), "s"(a.codes), "s"(a.n_frames),
                      "s"(a.frame_cap), "s"(a.next_table), "s"(a.h_out), "s"(a.ssq_out), "s"(a.xh_out), "s"(a.gamma_next),
                      "s"(a.talker_emb), "s"(a.temperature), "s"(a.forced), "s"(a.next_qkv), "s"(a.qkv_out), "s"(a.qkv_ld));
    Q3_TL(43);
    __shared__ float sv[4];
    __shared__ int si[4];
    const int r = a.row0 + blockIdx.x, tid = threadIdx.x;
    const int RT = a.R_total > 0 ? a.R_total : a.R;
    float best = -INFINITY;
    int bidx = 0x7fffffff;
    const float4* lg = (const float4*)(a.logits + (size_t)r * a.V);
    const int n4 = a.V / 4;
    float4 l0 = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY), l1 = l0;
    if (tid < n4) l0 = lg[tid];
    if (tid + 256 < n4) l1 = lg[tid + 256];
    const int nf_r = uniform_load(a.n_frames + r);   // independent of the arg-max: a scalar load beside the logits' vector loads
    float temperature = a.temperature;
    int top_k = a.top_k;
    int text_avail = 0;   // rows of streamed text the row has (feedback launch of an engine with a text reservation only)
    int held = 0;         // the row is held in this step (an engine with q3e_text_hold only): see CpArgmaxArgs::held
    if constexpr (SLOTS) {
        if (a.held) held = uniform_load(a.held + r);
        const SlotParams sp = uniform_slot(a.slots, r);
        temperature = sp.c_temp;
        top_k = sp.c_top_k;
        if (a.talker_emb && a.text_rows) text_avail = uniform_load(a.text_avail + r);
    }
    Q3_PH(0);
    {
        const float e[8] = {nan_as_inf(l0.x), nan_as_inf(l0.y), nan_as_inf(l0.z), nan_as_inf(l0.w),
                            nan_as_inf(l1.x), nan_as_inf(l1.y), nan_as_inf(l1.z), nan_as_inf(l1.w)};
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int idx = (j < 4 ? tid : tid + 256) * 4 + (j & 3);
            if (e[j] > best) {   // ascending index within a thread: strict > keeps the lowest index
                best = e[j];
                bidx = idx;
            }
        }
    }
    for (int v4 = tid + 512; v4 < n4; v4 += 256) {   // vocabularies beyond 2048
        const float4 l = lg[v4];
        const float e[4] = {nan_as_inf(l.x), nan_as_inf(l.y), nan_as_inf(l.z), nan_as_inf(l.w)};
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (e[j] > best) {
                best = e[j];
                bidx = v4 * 4 + j;
            }
    }
    group_argmax_down<64>(best, bidx);
    if ((tid & 63) == 0) {
        sv[tid >> 6] = best;
        si[tid >> 6] = bidx;
    }
    __syncthreads();
    Q3_PH(1);  // logits landed, wave arg-max done, barrier passed
    best = sv[0];
    bidx = si[0];
#pragma unroll
    for (int i = 1; i < 4; i++)
        if (sv[i] > best || (sv[i] == best && si[i] < bidx)) {
            best = sv[i];
            bidx = si[i];
        }
    const float sc_m = best;   // (SCORES) the maximum of the raw logits, before a draw replaces the winner
    float sc_sum = 0.f;
    if constexpr (SCORES) {
        __shared__ float sc_ws[4];
        const float e[8] = {nan_as_inf(l0.x), nan_as_inf(l0.y), nan_as_inf(l0.z), nan_as_inf(l0.w),
                            nan_as_inf(l1.x), nan_as_inf(l1.y), nan_as_inf(l1.z), nan_as_inf(l1.w)};
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; j++) s += expf(e[j] - sc_m);   // (a lane's padding is -inf: exp(-inf) = 0)
        for (int v4 = tid + 512; v4 < n4; v4 += 256) {         // vocabularies beyond 2048: read again
            const float4 l = lg[v4];
            s += expf(nan_as_inf(l.x) - sc_m);
            s += expf(nan_as_inf(l.y) - sc_m);
            s += expf(nan_as_inf(l.z) - sc_m);
            s += expf(nan_as_inf(l.w) - sc_m);
        }
        s = wave_sum(s);
        if ((tid & 63) == 0) sc_ws[tid >> 6] = s;
        __syncthreads();
        sc_sum = ((sc_ws[0] + sc_ws[1]) + sc_ws[2]) + sc_ws[3];
    }
    if (temperature > 1e-6f) {   // code_predictor_server.py:87-92: top-k, softmax((l-max)/T), categorical draw
        extern __shared__ float slg[];
        __shared__ float selv[64];
        __shared__ int seli[64];
        __shared__ float sv2[16];
        __shared__ int si2[16];
        __syncthreads();
        for (int v = tid; v < a.V; v += 256) slg[v] = nan_as_inf(a.logits[(size_t)r * a.V + v]);
        __syncthreads();
        float u;
        if constexpr (SLOTS) {
            const SlotParams sp = uniform_slot(a.slots, r);
            u = uniform01(sp.seed, sp.no_row ? 0u : (unsigned)r, (unsigned)nf_r, 1u + (unsigned)a.group);
        } else {
            u = uniform01(a.seed_ptr ? a.seed_ptr[r] : a.seed, (unsigned)r, (unsigned)nf_r, 1u + (unsigned)a.group);
        }
        float top_p = 0.f;   // no nucleus cut (code_predictor_server.py has none)
        if constexpr (RULES) top_p = uniform_rules(a.rules, r).cp_top_p;
        bidx = block_sample_topk(slg, a.V, top_k, temperature, top_p, u, sv2, si2, selv, seli);
    }
    if (bidx < 0 || bidx >= a.V) bidx = 0;   // every logit -inf: numpy's argmax answers 0; never gather with an invalid winner
    int f = nf_r - 1;
    if (f < 0) f = 0;
    const bool keep = f < a.frame_cap;        // a frame beyond the codes array is not recorded
    if (!keep) f = a.frame_cap - 1;
    int* fc = a.codes + ((size_t)f * RT + r) * 16;
    if (SLOTS && held) {   // (a held row has 1 <= n_frames <= frame_cap: its frame is recorded)
        bidx = fc[1 + a.group];
        if (bidx < 0 || bidx >= a.V) bidx = 0;
    } else if (tid == 0 && keep) fc[1 + a.group] = bidx;
    const int* fz = (a.forced && keep) ? a.forced + ((size_t)f * RT + r) * 16 : nullptr;
    if (fz && fz[1 + a.group] >= 0) bidx = fz[1 + a.group];   // teacher forcing (tests): continue with the forced id
    if constexpr (SCORES) {
        if (a.scores && tid == 0 && keep && !(SLOTS && held)) {   // where fc[1 + group] was written, of the id used
            const float zu = bidx >= 0 && bidx < a.V ? nan_as_inf(a.logits[(size_t)r * a.V + bidx]) : -INFINITY;
            // a maximum of +inf, or nothing above -inf: the formula's own inf - inf
            a.scores[((size_t)f * RT + r) * 16 + 1 + a.group] =
                (sc_m < INFINITY && sc_m > -INFINITY) ? zu - sc_m - logf(sc_sum) : __builtin_nanf("");
        }
    }
    Q3_PH(2);
    if (a.talker_emb) {
        // text slot: row f of the slot's text stands where the pad stands (f from the slot's own start, before the clamps
        // above; f < avail <= text_cap keeps the index inside the buffer, also for ended rows past frame_cap).  Uniform.
        const float* last = a.pad_embed;
        if constexpr (SLOTS)
            if (nf_r >= 1 && nf_r - 1 < text_avail) last = a.text_rows + ((size_t)r * a.text_cap + (nf_r - 1)) * a.H;
        feedback_row(fc, r, a.talker_emb, a.talker_vocab, a.cp_tables, a.V, a.n_groups, last,
                     a.h_out, a.ssq_out, a.H, a.group, bidx, fz, a.xh_out, a.gamma_next);
    } else if (a.next_table) {
        // a forced id beyond the vocabulary embeds as zeros (gather_embed_kernel's rule) and reads neither table; the
        // loads below are unconditional at a clamped index, so that none of them sits behind a branch of its own
        const bool ok = bidx < a.V;
        const int t = ok ? bidx : 0;
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        const float* erow = a.next_table + (size_t)t * a.H;
        const int ne4 = a.H / 4;
        if (a.next_qkv) {
            // layer 0's q|k|v of this token comes from the table of the group (a pure function of the token: cp_frame
            // launches no q|k|v GEMV for this pass): its loads go out together with the embedding row's, one round trip
            constexpr int QV = 4;                       // float4 per thread held in registers: 4096 columns
            const int nq4 = a.qkv_ld / 4;
            const float4* tq = (const float4*)(a.next_qkv + (size_t)t * a.qkv_ld);
            float4* dq = (float4*)(a.qkv_out + (size_t)r * a.qkv_ld);
            float4 ev = *(const float4*)(erow + (tid < ne4 ? tid : 0) * 4);
            float4 qv[QV];
#pragma unroll
            for (int j = 0; j < QV; j++) {
                const int i = tid + 256 * j;
                qv[j] = tq[i < nq4 ? i : 0];
            }
            if (!ok) {   // (uniform)
                ev = zero;
#pragma unroll
                for (int j = 0; j < QV; j++) qv[j] = zero;
            }
            if (tid < ne4) store_row_ssq(a.h_out, a.ssq_out, r, a.H, tid, ev, a.xh_out, a.gamma_next);
#pragma unroll
            for (int j = 0; j < QV; j++) {
                const int i = tid + 256 * j;
                if (i < nq4) dq[i] = qv[j];
            }
            for (int k4 = tid + 256; k4 < ne4; k4 += 256) {   // rows beyond 1024 / 4096 columns
                float4 v = *(const float4*)(erow + k4 * 4);
                if (!ok) v = zero;
                store_row_ssq(a.h_out, a.ssq_out, r, a.H, k4, v, a.xh_out, a.gamma_next);
            }
            for (int i = tid + 256 * QV; i < nq4; i += 256) {
                float4 v = tq[i];
                if (!ok) v = zero;
                dq[i] = v;
            }
        } else {
            for (int k4 = tid; k4 < ne4; k4 += 256) {
                float4 v = *(const float4*)(erow + k4 * 4);
                if (!ok) v = zero;
                store_row_ssq(a.h_out, a.ssq_out, r, a.H, k4, v, a.xh_out, a.gamma_next);
            }
        }
    }
}
__global__ void __launch_bounds__(256) cp_argmax_kernel(CpArgmaxArgs a) { cp_argmax_row<false>(a); }
__global__ void __launch_bounds__(256) cp_argmax_kernel_slots(CpArgmaxArgs a) { cp_argmax_row<true>(a); }
__global__ void __launch_bounds__(256) cp_argmax_kernel_rules(CpArgmaxArgs a) { cp_argmax_row<true, true>(a); }
__global__ void __launch_bounds__(256) cp_argmax_kernel_scores(CpArgmaxArgs a) { cp_argmax_row<false, false, true>(a); }
__global__ void __launch_bounds__(256) cp_argmax_kernel_slots_scores(CpArgmaxArgs a) { cp_argmax_row<true, false, true>(a); }
__global__ void __launch_bounds__(256) cp_argmax_kernel_rules_scores(CpArgmaxArgs a) { cp_argmax_row<true, true, true>(a); }

int launch_cp_argmax(hipStream_t s, const CpArgmaxArgs& a) {
    if (a.R <= 0) return 0;
    if (a.V % 4) {   // the arg-max reads each row as V / 4 float4: a tail would be dropped, and odd rows misaligned
        Q3_LOG("cp_argmax: a vocabulary of %d is not a multiple of 4", a.V);
        return -1;
    }
    // text rows and held rows are read in per-slot mode only; text_rows is indexed with text_avail and text_cap
    if (((a.text_rows || a.text_avail || a.held) && !a.slots) || (a.text_rows && (!a.text_avail || a.text_cap <= 0))) {
        Q3_LOG("cp_argmax: text_rows / text_avail / held need per-slot mode, text_rows needs text_avail and text_cap > 0 "
               "(text_rows %p, text_avail %p, text_cap %d, held %p, slots %p)", (const void*)a.text_rows,
               (const void*)a.text_avail, a.text_cap, (const void*)a.held, (const void*)a.slots);
        return -1;
    }
    if (a.rules && !a.slots) {
        Q3_LOG("cp_argmax: rules need per-slot mode (rules %p, slots %p)", (const void*)a.rules, (const void*)a.slots);
        return -1;
    }
    if (sample_vocab_refused("cp_argmax", a.slots != nullptr, a.V, a.temperature, a.top_k)) return -1;
    const size_t lds = a.slots ? sample_lds_bytes_slots(a.V) : sample_lds_bytes(a.V, a.top_k, a.temperature);
    CpArgmaxArgs a2 = a;
    a2.tl_node = tl_next_node();
    // [scores][plain | slots | rules] (q3e_scores_reserve: the same choice among the kernels that also score)
    static void (*const kernels[2][3])(CpArgmaxArgs) = {
        {cp_argmax_kernel, cp_argmax_kernel_slots, cp_argmax_kernel_rules},
        {cp_argmax_kernel_scores, cp_argmax_kernel_slots_scores, cp_argmax_kernel_rules_scores}};
    hipLaunchKernelGGL(kernels[a.scores ? 1 : 0][a.rules ? 2 : a.slots ? 1 : 0], dim3(a.R), dim3(256), lds, s, a2);
    Q3_HIP(hipGetLastError(), -1);
    return 0;
}

}  // namespace q3
