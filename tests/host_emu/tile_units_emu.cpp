// The cutters of ragged IMDCT and ISTFT batches (imdct_cut_units / istft_cut_units, zafx_units.hpp) on the host: prints the units one of them
// makes of one batch and the deal.
//     g++ -O2 -std=c++17 -I zaf-python_amd/csrc tests/host_emu/tile_units_emu.cpp -o tile_units_emu
//     ./tile_units_emu imdct tile_frames slots grid T0 T1 ...
//     ./tile_units_emu istft W H tile_frames slots grid T0 T1 ...    (frame counts may also come on standard input, one per token, after a lone "-")
// Output: "S <segment length in tiles>", [istft: one line "L clip samples" per spectrum (istft_out_len),] one line "U clip tile_a tile_b tiles T"
// per unit in the cutter's order, "G <workgroups of the launch>" = min(grid, units), then one line "D clip tile_a tile_b tiles T" per record of
// the table in launch order (deal_table; clip -1: a record without tiles).  istft: the units are filled in with tile_fill_clip at the pitch T
// rounded up to 16, and the U and D lines end with "out_len TP".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "zafx_units.hpp"

int main(int argc, char** argv) {
    if (argc < 2 || (std::strcmp(argv[1], "imdct") && std::strcmp(argv[1], "istft"))) return 2;
    const bool istft = argv[1][1] == 's';
    const int at = istft ? 4 : 2;   // where tile_frames, slots, grid and the frame counts begin
    if (argc < at + 3) return 2;
    const int W = istft ? std::atoi(argv[2]) : 0, H = istft ? std::atoi(argv[3]) : 0, tile_frames = std::atoi(argv[at]);
    const long long slots = std::atoll(argv[at + 1]);
    long long grid = std::atoll(argv[at + 2]);
    std::vector<int64_t> frames;
    if (argc == at + 4 && argv[at + 3][0] == '-' && argv[at + 3][1] == 0) {
        long long v;
        while (std::scanf("%lld", &v) == 1) frames.push_back(v);
    } else {
        for (int i = at + 3; i < argc; ++i) frames.push_back(std::atoll(argv[i]));
    }
    const int64_t n = (int64_t)frames.size();
    auto units = istft ? zafx::istft_cut_units(frames.data(), n, W, H, tile_frames, slots) : zafx::imdct_cut_units(frames.data(), n, tile_frames, slots);
    std::printf("S %lld\n", istft ? zafx::istft_segment_tiles(frames.data(), n, W, H, tile_frames, slots) : zafx::imdct_segment_tiles(frames.data(), n, tile_frames, slots));
    auto print = [istft](char tag, long long clip, const zafx::TileUnit& u) {
        std::printf("%c %lld %d %d %d %d", tag, clip, u.tile_a, u.tile_b, u.tiles, u.T);
        if (istft) std::printf(" %lld %d", u.out_len, u.TP);
        std::printf("\n");
    };
    if (istft) {
        for (size_t i = 0; i < frames.size(); ++i) std::printf("L %zu %lld\n", i, zafx::istft_out_len(frames[i], W, H));
        for (auto& u : units)   // (the cutter leaves the clip's index in in_off; the emulator keeps it there)
            zafx::tile_fill_clip(u, u.in_off, 0, (u.T + 15) / 16 * 16, zafx::istft_out_len(u.T, W, H));
    }
    for (const auto& u : units) print('U', u.in_off, u);
    grid = std::min(grid, (long long)units.size());
    const auto table = zafx::deal_table(units, grid);
    std::printf("G %lld\n", grid);
    for (const auto& u : table) print('D', u.tile_b > u.tile_a ? u.in_off : -1LL, u);
    return 0;
}
