// zafx_ragged_table.hpp -- the table of a ragged batch (zafx_execute_ragged): one record per clip, then the clip of every tile.
//
// A tile is `tile_frames` consecutive frames of ONE clip: 16 for k_stft_ft16 / k_mel2, 32 for k_mdct_ft32; float64: 8 for k_stft_ft8_f64,
// 16 for k_mdct_ft16_f64 / k_mel_ft8_f64.  A clip of T frames owns
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
#include <vector>

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

// zafx_execute_ragged_pcm, the batches no kernel reads as integers: the clip list cut, in the order given, into groups of consecutive clips
// whose covered span of the integer array -- sample frames [lo, hi): lowest offset to highest end -- converts into a float32 staging array of
// `budget_frames` samples.  A group has at least one clip, so a clip longer than the budget is a group of its own; clips whose offsets go
// back and forth cover more than the sum of their lengths and are cut into smaller groups, one clip each in the worst case.  Clip i of a
// group lies at offsets[i] - lo of the group's staging copy.  (An end past INT64_MAX saturates: such a clip is a group of its own.)
struct RgPcmGroup {
    long long first, count, lo, hi;
};

inline std::vector<RgPcmGroup> rg_pcm_groups(const int64_t* offsets, const int64_t* lengths, long long n_clips, long long budget_frames) {
    std::vector<RgPcmGroup> groups;
    auto end_of = [&](long long i) { return lengths[i] > INT64_MAX - offsets[i] ? (long long)INT64_MAX : (long long)(offsets[i] + lengths[i]); };
    for (long long i = 0; i < n_clips;) {
        RgPcmGroup g = {i, 1, (long long)offsets[i], end_of(i)};
        for (long long j = i + 1; j < n_clips; ++j) {
            const long long lo = std::min<long long>(g.lo, offsets[j]), hi = std::max(g.hi, end_of(j));
            if (hi - lo > budget_frames) break;
            g.lo = lo, g.hi = hi, ++g.count;
        }
        groups.push_back(g);
        i += g.count;
    }
    return groups;
}

}  // namespace zafx
