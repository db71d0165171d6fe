// zafx_ragged_table.hpp -- the table of a ragged batch (zafx_execute_ragged): one record per clip, then the clip of every tile.
//
// A tile is `tile_frames` consecutive frames of ONE clip: 16 for k_stft_ft16 / k_mel2, 32 for k_mdct_ft32.  A clip of T frames owns
// ceil(T / tile_frames) consecutive tiles from its first_tile on -- a clip of length 0 still has T >= 1 frame (zafx_plan_out_dims), so it
// owns one tile -- and the batch's tiles are numbered in clip order.  The kernels' RAGGED forms find a tile's clip in the per-tile array
// and everything else in the clip's record.
//
// Plain C++: compiled by hipcc into the library and by g++ into tests/host_emu/ragged_table_emu.cpp.
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>

namespace zafx {

// One clip of a ragged batch.  The plan's table on the device is n_clips of these, then one int per tile of the batch: the clip it
// belongs to.  Offsets and lengths in elements of the input / output arrays.
struct RgClip {
    long long in_off, n_samples, out_off;
    int T, TP, first_tile, pad_;
};
static_assert(sizeof(RgClip) == 40 && alignof(RgClip) == 8, "RgClip: the layout the host writes");

inline long long rg_tiles(long long frames, int tile_frames) { return (frames + tile_frames - 1) / tile_frames; }

// first_tile of every record for tiles of `tile_frames` frames; -> the batch's tiles.  (A batch of 2^31 tiles or more has no native launch:
// first_tile saturates, the caller checks the sum.)
inline long long rg_assign_tiles(RgClip* recs, size_t n_clips, int tile_frames) {
    long long tiles = 0;
    for (size_t c = 0; c < n_clips; ++c) {
        recs[c].first_tile = (int)std::min<long long>(tiles, INT_MAX);
        tiles += rg_tiles(recs[c].T, tile_frames);
    }
    return tiles;
}

// The per-tile part of the table: clip_of[first_tile + j] = c for the tiles j of clip c.
inline void rg_fill_clip_of(const RgClip* recs, size_t n_clips, int tile_frames, int* clip_of) {
    for (size_t c = 0; c < n_clips; ++c) {
        const long long tiles = rg_tiles(recs[c].T, tile_frames);
        for (long long j = 0; j < tiles; ++j) clip_of[recs[c].first_tile + j] = (int)c;
    }
}

}  // namespace zafx
