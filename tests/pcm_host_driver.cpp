// pcm_host_driver.cpp -- the host arithmetic of the encoder's PCM front-end (csrc/q3_enc_pcm_host.h) behind a command line,
// for tests/test_pcm_host.py.  The header is plain C++ and compiles alone: no HIP, no library.  Built once plain and once with
// -fsanitize=address,undefined; a stand-alone program, run on the CPU.
//
//   pcm_host_driver plan <format> <channels> <rate>        -> "plan up down half n_taps per_phase window256" or "refused"
//   pcm_host_driver clip <rate> <n_in> <max_samples>       -> "n_out N" or "refused"
//   pcm_host_driver taps <up> <down> <file>                -> the N taps as raw little-endian doubles into <file>, "taps N"
//   pcm_host_driver poly <up> <down> <file>                -> the [per_phase][up] device table into <file>, "poly J up"
//        (by factors, not by rate: no rate of 8000..192000 Hz reduces to a factor of exactly 640)
// Exit status 0 unless the arguments cannot be read (2).
#include "../qwen3_tts_axera_russian_amd/csrc/q3_enc_pcm_host.h"

#include <cstdlib>
#include <cstring>
#include <string>

using namespace q3;

static bool dump(const char* path, const std::vector<double>& v) {
    FILE* f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = fwrite(v.data(), sizeof(double), v.size(), f) == v.size();
    return fclose(f) == 0 && ok;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    EncPcmPlan p;
    if (cmd == "plan" && argc == 5) {
        if (!enc_pcm_plan(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), &p, "driver")) {
            puts("refused");
            return 0;
        }
        printf("plan %d %d %d %d %d %lld\n", p.up, p.down, p.half, p.n_taps, p.per_phase, enc_pcm_window(p, 256));
        return 0;
    }
    if (cmd == "clip" && argc == 5) {
        if (!enc_pcm_plan(0, 1, atoi(argv[2]), &p, "driver")) {
            puts("refused");
            return 0;
        }
        const int n = enc_pcm_clip_out(p, atoll(argv[3]), atoi(argv[4]), "driver", 0);
        if (n < 0)
            puts("refused");
        else
            printf("n_out %d\n", n);
        return 0;
    }
    if ((cmd == "taps" || cmd == "poly") && argc == 5) {
        if (!enc_pcm_plan_factors(atoi(argv[2]), atoi(argv[3]), &p)) {
            Q3_PCM_LOG("driver: factors %s/%s outside 1..%d", argv[2], argv[3], ENC_PCM_MAX_FACTOR);
            puts("refused");
            return 0;
        }
        std::vector<double> h, t;
        enc_pcm_taps(p, h);
        if (cmd == "taps") {
            if (!dump(argv[4], h)) return 2;
            printf("taps %zu\n", h.size());
        } else {
            enc_pcm_polyphase(p, h, t);
            if (!dump(argv[4], t)) return 2;
            printf("poly %d %d\n", p.per_phase, p.up);
        }
        return 0;
    }
    return 2;
}
