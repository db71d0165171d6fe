// zafx_center_units.hpp -- a ragged stereo batch cut into the units k_center's RAGGED form walks (zafx_center.hip, zafx_execute_center_ragged).
//
// One unit = blocks [b0, b1) of one clip (a block is H = W / 2 sample frames), started by a halo frame, so it gives the same bits wherever
// it starts.  Rule: one segment length S in blocks for the whole batch,
//     S = max(4 F - 3, ceil(total blocks / (kCenterUnitsPerSlot x workgroup slots)));
// a clip of at most S blocks is one unit, a longer one is cut into ceil(n / S) near-equal segments (they differ by at most one block);
// a clip of length 0 gives no unit.  With S >= 4 F - 3 = 2 (2 F - 1) - 1 every segment of a cut clip keeps at least 2 F - 1 blocks -- two
// tiles of F frames, the floor of the equal-length launch: each segment pays one halo frame -- and none exceeds S.  The units are ordered by
// descending block count (ties: clip order, then b0): the kernel deals them out in rounds of gridDim.x neighbours in that order, forwards
// and backwards in turn, so the workgroups' sums stay within about one unit of each other.  A fixed deal: nothing is claimed at run time.
//
// Plain C++: compiled by hipcc into the library and by g++ into tests/host_emu/center_units_emu.cpp.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace zafx {

// One record of the device table.  Offsets and lengths in sample frames (one sample frame = 8 bytes: L, R).
struct CenterUnit {
    long long in_off, n_samples, out_off;   // the unit's CLIP: its first sample frame in the input, its length, its first sample frame in the output
    int b0, b1;                             // the unit: blocks [b0, b1) of that clip
};
static_assert(sizeof(CenterUnit) == 32 && alignof(CenterUnit) == 8, "CenterUnit: the layout the host writes");

constexpr int kCenterUnitsPerSlot = 12;   // units per workgroup slot the segment length aims at (where the batch has the blocks); measured: DESIGN.md 4.7

inline long long center_blocks(long long n_samples, int W) { return (n_samples + W / 2 - 1) / (W / 2); }

// The batch's segment length in blocks.
inline long long center_segment_blocks(const int64_t* lengths, int64_t n_clips, int W, int F, long long slots, int per_slot = kCenterUnitsPerSlot) {
    long long total = 0;
    for (int64_t i = 0; i < n_clips; ++i) total += center_blocks(lengths[i], W);
    const long long want = std::max<long long>(1, slots) * std::max(1, per_slot);
    return std::max<long long>(4LL * F - 3, (total + want - 1) / want);
}

// in_offsets / out_offsets: null = 0 for every clip.
inline std::vector<CenterUnit> center_cut_units(const int64_t* lengths, const int64_t* in_offsets, const int64_t* out_offsets, int64_t n_clips, int W,
                                                int F, long long slots, int per_slot = kCenterUnitsPerSlot) {
    const long long S = center_segment_blocks(lengths, n_clips, W, F, slots, per_slot);
    std::vector<CenterUnit> units;
    for (int64_t i = 0; i < n_clips; ++i) {
        const long long n = center_blocks(lengths[i], W);
        if (n <= 0) continue;
        const long long k = (n + S - 1) / S, q = n / k, r = n % k;   // r segments of q + 1 blocks, then k - r of q
        long long b = 0;
        for (long long j = 0; j < k; ++j) {
            const long long len = q + (j < r ? 1 : 0);
            units.push_back({in_offsets ? (long long)in_offsets[i] : 0LL, (long long)lengths[i], out_offsets ? (long long)out_offsets[i] : 0LL, (int)b,
                             (int)(b + len)});
            b += len;
        }
    }
    std::stable_sort(units.begin(), units.end(), [](const CenterUnit& a, const CenterUnit& b) { return a.b1 - a.b0 > b.b1 - b.b0; });
    return units;
}

}  // namespace zafx
