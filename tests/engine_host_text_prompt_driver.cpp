// engine_host_text_prompt_driver.cpp -- the slot book (csrc/q3_engine_host.h) for text slots that continue a codec prompt,
// beside the DEVICE's rule for the same slots, for tests/test_engine_host_text_prompt.py.  tests/engine_host_driver.cpp's
// slot events, with the prompt's length at admit; every step of `run` is also taken by a stand-in for the sampler's
// counters (talker_sample_row<true> of csrc/q3_sample.hip, as its contract in csrc/q3_kernels.h words it): n_past starts
// at the prompt's length, the budget the device sees is prompt + budget, and a row is held when it is a text slot before
// its final push, has not ended, n_past < its budget and g = n_past - prompt satisfies g >= 1 and g >= the rows pushed.
//
//   open B hold [max_frames]     q3e_text_hold(hold) + q3e_open(B) of an engine created with max_frames (default 64)
//   admit b budget text prompt   q3e_admit_prompted of one utterance (text: 1 = a text slot; prompt: T frames)
//   push b n final               q3e_push_text
//   run n                        q3e_run(n)
//   ended b                      q3e_get_done found slot b ended
//   release b                    q3e_release
//     -> "slots <room> <steps> | <age> <held> <starved> <held_next> <generated> <device held> | ..."  the first four as
//        tests/engine_host_driver.cpp prints them; generated: SlotBook::generated of the stand-in's n_past; device held: the
//        steps the stand-in held the row for since its admission
#include "../qwen3_tts_axera_russian_amd/csrc/q3_engine_host.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

struct Row {   // what the sampler reads and writes of one row
    int n_past = 0, prompt = 0, max_frames = 0, avail = 0, flags = 0, done = 1;
    long long held = 0;
};

int main() {
    q3::SlotBook book;
    std::vector<Row> dev;
    bool hold = false;
    int max_frames = 64;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string ev;
        if (!(in >> ev)) continue;
        long long a = 0, b = 0, c = 0, d = 0;
        in >> a >> b >> c >> d;
        int room = -1, steps = 0;
        if (ev == "open") {
            book.open((int)a);
            dev.assign((size_t)a, Row());
            hold = b != 0;
            max_frames = c > 0 ? (int)c : 64;
        } else if (ev == "admit") {
            book.admit((int)a, (int)b, c != 0, (int)d);
            Row r;
            r.n_past = r.prompt = (int)d;
            r.max_frames = (int)d + (int)b;   // (admit_slots: the device counts the prompt's frames with the emitted ones)
            r.flags = c != 0 ? 3 : 0;
            r.done = 0;
            dev[a] = r;
        } else if (ev == "push") {
            book.push((int)a, (int)b, c != 0);
            dev[a].avail += (int)b;
            if (c != 0) dev[a].flags = 1;
        } else if (ev == "ended") {
            book.mark_ended((int)a);
        } else if (ev == "release") {
            book.release((int)a);
            dev[a].done = 1;
            dev[a].avail = 0;
        } else if (ev == "run") {
            room = std::max(0, book.room(hold, max_frames));
            steps = std::min((int)a, room);
            book.advance(steps, hold, max_frames);
            for (int i = 0; i < steps; i++)
                for (Row& r : dev) {
                    const int g = r.n_past - r.prompt;
                    if (hold && (r.flags & 3) == 3 && !r.done && g >= 1 && g >= r.avail && r.n_past < r.max_frames) r.held++;
                    else if (!r.done && r.n_past >= r.max_frames) r.done = 1;
                    else if (!r.done) r.n_past++;
                }
        } else {
            fprintf(stderr, "unknown event: %s\n", line.c_str());
            return 2;
        }
        if (room < 0) room = std::max(0, book.room(hold, max_frames));
        printf("slots %d %d", room, steps);
        for (int s = 0; s < book.size(); s++)
            printf(" | %d %lld %d %d %d %lld", book[s].age, book[s].held, (int)book.starved(s), (int)(hold && book.held_next(s)),
                   book.generated(s, dev[s].n_past), dev[s].held);
        printf("\n");
    }
    return 0;
}
