// The tile table of a ragged batch (zafx_ragged_table.hpp) on the host: prints what zafx_execute_ragged uploads for one batch.
//     g++ -O2 -std=c++17 -I zaf-python_amd/csrc tests/host_emu/ragged_table_emu.cpp -o ragged_table_emu
//     ./ragged_table_emu tile_frames T0 T1 ...       (the clips' frame counts)
// Output: "tiles <n>", then "first <first_tile of every clip>", then "clip_of <clip of every tile>".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "zafx_ragged_table.hpp"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const int tile_frames = std::atoi(argv[1]);
    std::vector<zafx::RgClip> recs;
    for (int i = 2; i < argc; ++i) {
        zafx::RgClip r{};
        r.T = std::atoi(argv[i]);
        recs.push_back(r);
    }
    const long long tiles = zafx::rg_assign_tiles(recs.data(), recs.size(), tile_frames);
    std::vector<int> clip_of((size_t)tiles, -1);
    zafx::rg_fill_clip_of(recs.data(), recs.size(), tile_frames, clip_of.data());
    std::printf("tiles %lld\nfirst", tiles);
    for (const auto& r : recs) std::printf(" %d", r.first_tile);
    std::printf("\nclip_of");
    for (int c : clip_of) std::printf(" %d", c);
    std::printf("\n");
    return 0;
}
