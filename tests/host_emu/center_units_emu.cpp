// The cutter of ragged stereo batches (center_cut_units, zafx_units.hpp) on the host: prints the units it makes of one batch.
//     g++ -O2 -std=c++17 -I zaf-python_amd/csrc tests/host_emu/center_units_emu.cpp -o center_units_emu
//     ./center_units_emu W F slots len0 len1 ...        (lengths may also come on standard input, one per token, after a lone "-")
// Output: "S <segment length in blocks>", then one line "clip b0 b1 n_samples" per unit, in the order the kernel walks them.  The clip's index
// rides in the record's in_off, twice the index in its out_off.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "zafx_units.hpp"

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const int W = std::atoi(argv[1]), F = std::atoi(argv[2]);
    const long long slots = std::atoll(argv[3]);
    std::vector<int64_t> lengths, ids, ids2;
    if (argc == 5 && argv[4][0] == '-' && argv[4][1] == 0) {
        long long v;
        while (std::scanf("%lld", &v) == 1) lengths.push_back(v);
    } else {
        for (int i = 4; i < argc; ++i) lengths.push_back(std::atoll(argv[i]));
    }
    for (size_t i = 0; i < lengths.size(); ++i) ids.push_back((int64_t)i), ids2.push_back(2 * (int64_t)i);
    const auto units = zafx::center_cut_units(lengths.data(), ids.data(), ids2.data(), (int64_t)lengths.size(), W, F, slots);
    std::printf("S %lld\n", zafx::center_segment_blocks(lengths.data(), (int64_t)lengths.size(), W, F, slots));
    for (const auto& u : units) {
        if (u.out_off != 2 * u.in_off) return 3;
        std::printf("%lld %d %d %lld\n", u.in_off, u.b0, u.b1, u.n_samples);
    }
    return 0;
}
