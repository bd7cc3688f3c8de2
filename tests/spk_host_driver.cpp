// spk_host_driver.cpp -- the host arithmetic of the speaker encoder (csrc/q3_spk.h, the part outside its device section)
// behind a command line, for tests/test_spk_host.py.  Plain C++: no HIP, no library.  Built once plain and once with
// -fsanitize=address,undefined; a stand-alone program, run on the CPU.
//
//   spk_host_driver frames <n_fft> <hop> <pad> <min_frames> <n>   -> "frames F" or "refused"
//   spk_host_driver min <n_fft> <hop> <pad> <min_frames>          -> "min N"
//   spk_host_driver reflect <L> <lo> <hi>                         -> "reflect" and reflect(i, L) for i in lo..hi
// Exit status 0 unless the arguments cannot be read (2).
#include "../qwen3_tts_axera_russian_amd/csrc/q3_spk.h"

#include <cstdio>
#include <cstdlib>
#include <string>

using namespace q3;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    if (cmd == "frames" && argc == 7) {
        const int f = spk_frames_of(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoll(argv[6]));
        if (f < 0)
            puts("refused");
        else
            printf("frames %d\n", f);
        return 0;
    }
    if (cmd == "min" && argc == 6) {
        printf("min %d\n", spk_min_samples_of(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5])));
        return 0;
    }
    if (cmd == "reflect" && argc == 5) {
        printf("reflect");
        for (int i = atoi(argv[3]); i <= atoi(argv[4]); i++) printf(" %d", spk_reflect(i, atoi(argv[2])));
        putchar('\n');
        return 0;
    }
    return 2;
}
