// q3_engine_host.h -- the host-side rules of the per-slot engine (q3_engine.hip), without anything of HIP: which slots a
// frame step waits for, how many steps q3e_run may take and what they do to the slots' counters (SlotBook), and which
// entry of the prefix cache an admission hits, fills or evicts (PrefixIndex).  The contract is include/qwen3tts_engine.h
// (q3e_run, q3e_text_hold, q3e_text_state, q3e_prefix_cache); tests/engine_host_driver.cpp runs these rules on a CPU.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace q3 {

struct Slot {
    int budget = 0;        // frame budget of the utterance
    int age = -1;          // frames it has emitted (the steps since its admission it was not held for), capped at the
                           // engine's max_frames; < 0: the slot never held an utterance
    int text_rows = 0;     // rows pushed (text slots)
    long long held = 0;    // steps it was held for since its admission
    bool live = false;     // admitted and neither released nor known to have ended
    bool text = false;     // a text slot ...
    bool text_final = false;   // ... whose text has ended
    int prompt = 0;        // codec-prompt frames it was admitted with (q3e_admit_prompted): the device's n_past counts them,
                           // budget and age do not
};

class SlotBook {
public:
    void open(int B) { s_.assign(B, Slot()); }
    int size() const { return (int)s_.size(); }
    const Slot& operator[](int b) const { return s_[b]; }

    void admit(int b, int budget, bool is_text, int prompt = 0) { s_[b] = Slot{budget, 0, 0, 0, true, is_text, false, prompt}; }
    // frames slot b has generated, from the device's n_past (which starts at the prompt's length)
    int generated(int b, int n_past) const { return n_past - s_[b].prompt; }
    void release(int b) { s_[b].live = false; }
    void mark_ended(int b) { s_[b].live = false; }   // q3e_get_done saw its EOS or its whole budget
    void push(int b, int n, bool final) {
        s_[b].text_rows += n;
        if (final) s_[b].text_final = true;
    }

    // a live text slot whose text has not ended and that has budget left: its next frames need rows
    bool waits(int b) const {
        const Slot& s = s_[b];
        return s.live && s.text && !s.text_final && s.age < s.budget;
    }
    // the next step waits for slot b (q3e_text_state, in either mode)
    bool starved(int b) const { return waits(b) && s_[b].text_rows <= s_[b].age; }
    // q3e_text_hold: the device's verdict for slot b at its next step (talker_sample_row<true>) -- starved with a frame of
    // its own to repeat
    bool held_next(int b) const { return starved(b) && s_[b].age >= 1; }
    bool live_text(int b) const { return s_[b].live && s_[b].text; }
    int first_live_text() const {   // -1: none
        for (int b = 0; b < size(); b++)
            if (live_text(b)) return b;
        return -1;
    }

    // Steps q3e_run may take (<= 0: none).  Without hold: the most budget a live slot has left, but no step whose frame a
    // waiting slot has no row for.  With hold: the most steps a live slot can still use -- up to its rows (or its budget)
    // for a waiting slot, its budget for any other; 0 when every live slot is held, and 0 while a waiting slot has neither
    // a frame nor a row (nothing of its own to repeat: it stalls the batch).
    int room(bool hold, int max_frames) const {
        int most = 0, rows_left = max_frames;
        for (int b = 0; b < size(); b++) {
            const Slot& s = s_[b];
            if (!s.live) continue;
            int upto = s.budget;
            if (waits(b) && hold) {
                if (s.age == 0 && s.text_rows == 0) return 0;
                upto = std::min(s.text_rows, s.budget);
            } else if (waits(b)) {
                rows_left = std::min(rows_left, s.text_rows - s.age);
            }
            most = std::max(most, upto - s.age);
        }
        return hold ? most : std::min(most, rows_left);
    }

    // `steps` frame steps were taken.  Without hold every slot that ever held an utterance ages by them; with hold step by
    // step as the device decided (no row arrives during a run, so a slot that is held stays held for the rest of it).
    void advance(int steps, bool hold, int max_frames) {
        for (int b = 0; b < size(); b++) {
            Slot& s = s_[b];
            if (s.age < 0) continue;
            for (int i = 0; i < steps; i++) {
                if (hold && held_next(b)) {
                    s.held += steps - i;
                    break;
                }
                s.age = std::min(s.age + 1, max_frames);
            }
        }
    }

    // frames of the slot admitted longest ago: the rows q3e_get_codes returns
    int frames_hi() const {
        int hi = 0;
        for (const Slot& s : s_) hi = std::max(hi, s.age);
        return hi;
    }

private:
    std::vector<Slot> s_;
};

// Keys and use order of the prefix cache's entries (the device pool itself belongs to the engine).
class PrefixIndex {
public:
    enum Outcome { NOT_KEYED, HIT, MISS, TOO_LONG, NO_POOL };
    struct Lookup {
        Outcome what;
        int entry;   // HIT: the entry that holds the prefix; MISS: the entry that holds the key with another n_rows, or -1
    };
    long long hits = 0, misses = 0, stores = 0, evictions = 0, too_long = 0;   // (run on over resize)

    void resize(int n_entries, int max_rows) {
        e_.assign(n_entries, Entry());
        max_rows_ = max_rows;
    }
    int size() const { return (int)e_.size(); }
    int max_rows() const { return max_rows_; }
    int used() const {
        int n = 0;
        for (const Entry& p : e_) n += p.n_rows ? 1 : 0;
        return n;
    }

    // The admit loop: lookup; on a HIT restore from the entry, then hit(); otherwise prefill, then miss(), and store() into
    // the entry it names, if any.  lookup says what an admission of n_rows rows under (k0, k1) is and changes nothing; the
    // counters move in hit() / miss() / store(), after the launches they count are queued.
    Lookup lookup(uint64_t k0, uint64_t k1, int n_rows) const {
        if (k0 == 0 && k1 == 0) return {NOT_KEYED, -1};
        if (size() == 0) return {NO_POOL, -1};
        if (n_rows > max_rows_) return {TOO_LONG, -1};
        const int at = find(k0, k1);
        return {at >= 0 && e_[at].n_rows == n_rows ? HIT : MISS, at};
    }
    void hit(const Lookup& l) {
        e_[l.entry].use = ++clock_;
        hits++;
    }
    // Counts the admission and returns the entry to store it into -- the one that holds its key with another length, else
    // victim() -- freed (an entry whose store fails holds nothing); -1: nothing to store.
    int miss(const Lookup& l) {
        if (l.what == NOT_KEYED) return -1;
        too_long += l.what == TOO_LONG;
        misses += l.what != TOO_LONG;
        if (l.what != MISS) return -1;
        const int at = l.entry >= 0 ? l.entry : victim();
        e_[at].n_rows = 0;
        return at;
    }
    void store(int i, uint64_t k0, uint64_t k1, int n_rows) {
        e_[i] = Entry{k0, k1, n_rows, ++clock_};
        stores++;
    }

private:
    struct Entry {
        uint64_t k0 = 0, k1 = 0;
        int n_rows = 0;                // 0: free
        unsigned long long use = 0;    // clock_ of the last hit or store
    };
    int find(uint64_t k0, uint64_t k1) const {
        for (int i = 0; i < size(); i++)
            if (e_[i].n_rows && e_[i].k0 == k0 && e_[i].k1 == k1) return i;
        return -1;
    }
    // the first free entry, else the least recently used one, which counts as an eviction
    int victim() {
        int at = 0;
        for (int i = 0; i < size() && e_[at].n_rows; i++)
            if (!e_[i].n_rows || e_[i].use < e_[at].use) at = i;
        evictions += e_[at].n_rows != 0;
        return at;
    }
    std::vector<Entry> e_;
    unsigned long long clock_ = 0;
    int max_rows_ = 0;
};

}  // namespace q3
