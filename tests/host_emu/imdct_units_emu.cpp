// The cutter of ragged IMDCT batches (imdct_cut_units, zafx_units.hpp) on the host: prints the units it makes of one batch and the deal.
//     g++ -O2 -std=c++17 -I zaf-python_amd/csrc tests/host_emu/imdct_units_emu.cpp -o imdct_units_emu
//     ./imdct_units_emu tile_frames slots grid T0 T1 ...        (frame counts may also come on standard input, one per token, after a lone "-")
// Output: "S <segment length in tiles>", one line "U clip tile_a tile_b tiles T" per unit in the cutter's order, "G <workgroups of the launch>" =
// min(grid, units), then one line "D clip tile_a tile_b tiles T" per record of the table in launch order (deal_table; clip -1: a record
// without tiles).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "zafx_units.hpp"

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const int tile_frames = std::atoi(argv[1]);
    const long long slots = std::atoll(argv[2]);
    long long grid = std::atoll(argv[3]);
    std::vector<int64_t> frames;
    if (argc == 5 && argv[4][0] == '-' && argv[4][1] == 0) {
        long long v;
        while (std::scanf("%lld", &v) == 1) frames.push_back(v);
    } else {
        for (int i = 4; i < argc; ++i) frames.push_back(std::atoll(argv[i]));
    }
    const auto units = zafx::imdct_cut_units(frames.data(), (int64_t)frames.size(), tile_frames, slots);
    std::printf("S %lld\n", zafx::imdct_segment_tiles(frames.data(), (int64_t)frames.size(), tile_frames, slots));
    for (const auto& u : units) std::printf("U %lld %d %d %d %d\n", u.in_off, u.tile_a, u.tile_b, u.tiles, u.T);
    grid = std::min(grid, (long long)units.size());
    const auto table = zafx::deal_table(units, grid);
    std::printf("G %lld\n", grid);
    for (const auto& u : table) std::printf("D %lld %d %d %d %d\n", u.tile_b > u.tile_a ? u.in_off : -1LL, u.tile_a, u.tile_b, u.tiles, u.T);
    return 0;
}
