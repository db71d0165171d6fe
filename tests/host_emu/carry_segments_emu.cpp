// carry_segments (zafx_units.hpp), the cut of an equal-length batch's clips into segments for the carry kernels, on the host.
//     g++ -O2 -std=c++17 -I zaf-python_amd/csrc tests/host_emu/carry_segments_emu.cpp -o carry_segments_emu
//     ./carry_segments_emu grid max_clips max_tiles     one line "n_clips tiles segs" for every n_clips in 1..max_clips and tiles in 1..max_tiles
//     ./carry_segments_emu grid = n_clips tiles         that one line
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "zafx_units.hpp"

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const long long grid = std::atoll(argv[1]);
    if (grid < 1) return 2;
    if (!std::strcmp(argv[2], "=")) {
        if (argc < 5) return 2;
        const long long n = std::atoll(argv[3]);
        const int t = std::atoi(argv[4]);
        std::printf("%lld %d %d\n", n, t, zafx::carry_segments(n, t, grid));
        return 0;
    }
    const long long max_clips = std::atoll(argv[2]);
    const int max_tiles = std::atoi(argv[3]);
    for (long long n = 1; n <= max_clips; ++n)
        for (int t = 1; t <= max_tiles; ++t) std::printf("%lld %d %d\n", n, t, zafx::carry_segments(n, t, grid));
    return 0;
}
