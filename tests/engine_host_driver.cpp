// engine_host_driver.cpp -- the engine's host rules (csrc/q3_engine_host.h) behind a line protocol, for
// tests/test_engine_host.py.  Every event does what the entry point of include/qwen3tts_engine.h named beside it does to
// the slot book or the prefix index, and answers with one line.
//
//   open B hold [max_frames]   q3e_text_hold(hold) + q3e_open(B) of an engine created with max_frames (default 64)
//   admit b budget text        q3e_admit of one utterance (text: 1 = a text slot)
//   push b n final             q3e_push_text
//   run n                      q3e_run(n)
//   ended b                    q3e_get_done found slot b ended
//   release b                  q3e_release
//     -> "slots <room> <steps> | <age> <held> <starved> <held_next> | ..."  room: the steps q3e_run may take now (for `run`:
//        the room it had), steps: the steps `run` took; then every slot: frames emitted, steps held, q3e_text_state's
//        starved, and whether the next step would hold it
//   pfx n_entries max_rows     q3e_prefix_cache
//   key k0 k1 n_rows           q3e_admit_keyed of one utterance
//     -> "pfx <class> <entry> <hits> <misses> <stores> <evictions> <too long> <used>"  class: - (pfx event), unkeyed, hit, miss,
//        too_long, no_pool; entry: the entry restored from or stored into, else -1
#include "../qwen3_tts_axera_russian_amd/csrc/q3_engine_host.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

int main() {
    q3::SlotBook book;
    q3::PrefixIndex pfx;
    bool hold = false;
    int max_frames = 64;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string ev;
        if (!(in >> ev)) continue;
        long long a = 0, b = 0, c = 0;
        unsigned long long k0 = 0, k1 = 0;
        if (ev == "key") in >> k0 >> k1 >> a;
        else in >> a >> b >> c;
        if (ev == "pfx" || ev == "key") {
            const char* what = "-";
            int entry = -1;
            if (ev == "pfx") {
                pfx.resize((int)a, a > 0 ? (int)b : 0);
            } else {
                static const char* names[] = {"unkeyed", "hit", "miss", "too_long", "no_pool"};
                const q3::PrefixIndex::Lookup l = pfx.lookup(k0, k1, (int)a);
                what = names[l.what];
                if (l.what == q3::PrefixIndex::HIT) {
                    pfx.hit(l);
                    entry = l.entry;
                } else if ((entry = pfx.miss(l)) >= 0) {
                    pfx.store(entry, k0, k1, (int)a);
                }
            }
            printf("pfx %s %d %lld %lld %lld %lld %lld %d\n", what, entry, pfx.hits, pfx.misses, pfx.stores, pfx.evictions,
                   pfx.too_long, pfx.used());
            continue;
        }
        int room = -1, steps = 0;
        if (ev == "open") {
            book.open((int)a);
            hold = b != 0;
            max_frames = c > 0 ? (int)c : 64;
        } else if (ev == "admit") {
            book.admit((int)a, (int)b, c != 0);
        } else if (ev == "push") {
            book.push((int)a, (int)b, c != 0);
        } else if (ev == "ended") {
            book.mark_ended((int)a);
        } else if (ev == "release") {
            book.release((int)a);
        } else if (ev == "run") {
            room = std::max(0, book.room(hold, max_frames));
            steps = std::min((int)a, room);
            book.advance(steps, hold, max_frames);
        } else {
            fprintf(stderr, "unknown event: %s\n", line.c_str());
            return 2;
        }
        if (room < 0) room = std::max(0, book.room(hold, max_frames));
        printf("slots %d %d", room, steps);
        for (int s = 0; s < book.size(); s++)
            printf(" | %d %lld %d %d", book[s].age, book[s].held, (int)book.starved(s), (int)(hold && book.held_next(s)));
        printf("\n");
    }
    return 0;
}
