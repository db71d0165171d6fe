// The cutter of ragged ISTFT batches (istft_cut_units, zafx_units.hpp) on the host: prints the units it makes of one batch and the deal.
//     g++ -O2 -std=c++17 -I zaf-python_amd/csrc tests/host_emu/istft_units_emu.cpp -o istft_units_emu
//     ./istft_units_emu W H tile_frames slots grid T0 T1 ...    (frame counts may also come on standard input, one per token, after a lone "-")
// Output: "S <segment length in tiles>", one line "L clip samples" per spectrum (istft_out_len), one line "U clip tile_a tile_b tiles T out_len TP"
// per unit in the cutter's order (filled in with istft_fill_clip at the pitch T rounded up to 16), "G <workgroups of the launch>" =
// min(grid, units), then one line "D clip tile_a tile_b tiles T out_len TP" per record of the table in launch order (deal_table; clip -1: a
// record without tiles).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "zafx_units.hpp"

int main(int argc, char** argv) {
    if (argc < 6) return 2;
    const int W = std::atoi(argv[1]), H = std::atoi(argv[2]), tile_frames = std::atoi(argv[3]);
    const long long slots = std::atoll(argv[4]);
    long long grid = std::atoll(argv[5]);
    std::vector<int64_t> frames;
    if (argc == 7 && argv[6][0] == '-' && argv[6][1] == 0) {
        long long v;
        while (std::scanf("%lld", &v) == 1) frames.push_back(v);
    } else {
        for (int i = 6; i < argc; ++i) frames.push_back(std::atoll(argv[i]));
    }
    auto units = zafx::istft_cut_units(frames.data(), (int64_t)frames.size(), W, H, tile_frames, slots);
    std::printf("S %lld\n", zafx::istft_segment_tiles(frames.data(), (int64_t)frames.size(), W, H, tile_frames, slots));
    for (size_t i = 0; i < frames.size(); ++i) std::printf("L %zu %lld\n", i, zafx::istft_out_len(frames[i], W, H));
    for (auto& u : units) {   // (the cutter leaves the clip's index in in_off; the emulator keeps it there)
        const long long clip = u.in_off;
        zafx::istft_fill_clip(u, clip, 0, (u.T + 15) / 16 * 16, W, H);
        std::printf("U %lld %d %d %d %d %lld %d\n", u.in_off, u.tile_a, u.tile_b, u.tiles, u.T, u.out_len, u.TP);
    }
    grid = std::min(grid, (long long)units.size());
    const auto table = zafx::deal_table(units, grid);
    std::printf("G %lld\n", grid);
    for (const auto& u : table)
        std::printf("D %lld %d %d %d %d %lld %d\n", u.tile_b > u.tile_a ? u.in_off : -1LL, u.tile_a, u.tile_b, u.tiles, u.T, u.out_len, u.TP);
    return 0;
}
