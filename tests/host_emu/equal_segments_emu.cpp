// center_equal_segments and maskfilter_equal_segments (zafx_units.hpp), the cut of an equal-length batch's clips into segments for k_center,
// k_maskfilter and k_maskfilter_stems, on the host.
//     g++ -O2 -std=c++17 -I zaf-python_amd/csrc tests/host_emu/equal_segments_emu.cpp -o equal_segments_emu
//     ./equal_segments_emu center|maskfilter F slots n_clips n_blocks [n_clips n_blocks ...]     one line "seg_blocks segs" for every pair
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "zafx_units.hpp"

int main(int argc, char** argv) {
    if (argc < 6 || (argc - 4) % 2) return 2;
    const bool center = !std::strcmp(argv[1], "center");
    if (!center && std::strcmp(argv[1], "maskfilter")) return 2;
    const int F = std::atoi(argv[2]);
    const long long slots = std::atoll(argv[3]);
    if (F < 1 || slots < 1) return 2;
    for (int i = 4; i + 1 < argc; i += 2) {
        const long long n_clips = std::atoll(argv[i]), n_blocks = std::atoll(argv[i + 1]);
        if (n_clips < 1 || n_blocks < 1) return 2;
        const zafx::EqualSegments s = center ? zafx::center_equal_segments(n_blocks, n_clips, F, slots) : zafx::maskfilter_equal_segments(n_blocks, n_clips, F, slots);
        std::printf("%lld %lld\n", (long long)s.seg_blocks, s.segs);
    }
    return 0;
}
