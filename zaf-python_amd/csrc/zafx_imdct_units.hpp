// zafx_imdct_units.hpp -- a ragged batch of MDCT coefficient blocks cut into the units k_imdct's RAGGED form walks (zafx_mdct.hip,
// zafx_execute_imdct_ragged).
//
// One unit = tiles [tile_a, tile_b) of one clip (a tile is `tile_frames` consecutive frames); a unit that does not start its clip first runs
// the tile in front of it in carry-only mode, so it gives the same bits wherever it starts.  Rule: one segment length S in
// tiles for the whole batch,
//     S = max(3, ceil(total tiles / (kImdctUnitsPerSlot x workgroup slots)));
// a clip of at most S tiles is one unit, a longer one is cut into ceil(n / S) near-equal segments (they differ by at most one tile); a clip
// whose output is empty (T <= 1: the reference returns y[M : -M-1], max(M (T - 1) - 1, 0) samples) gives no unit.  The floor of S is 3 =
// 2 x 2 - 1, not 2: every segment of a cut clip is to keep at least two tiles -- each pays one carry-only tile -- and none may exceed S, and a
// clip of 3 tiles against S = 2 can do neither (with S >= 3 and n > S, 2 ceil(n / S) <= n).  The units are ordered by descending tile count
// (ties: clip order, then tile_a) and dealt in rounds of `grid` neighbours in that order, forwards and backwards in turn (imdct_deal_table), so
// the workgroups' sums stay within about one unit of each other.  A fixed deal: nothing is claimed at run time.
//
// Plain C++: compiled by hipcc into the library and by g++ into tests/host_emu/imdct_units_emu.cpp.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace zafx {

// One record of the device table.  Offsets and lengths in floats.
struct ImdctUnit {
    long long in_off, out_off, out_len;   // the unit's CLIP: its block in the coefficient array, its first sample in the output, its samples M (T - 1) - 1
    int T, TP, tiles;                     // ... its frames, the pitch of its M rows, its tiles
    int tile_a, tile_b, pad_;             // the unit: tiles [tile_a, tile_b) of that clip
};
static_assert(sizeof(ImdctUnit) == 48 && alignof(ImdctUnit) == 8, "ImdctUnit: the layout the host writes");

constexpr int kImdctUnitsPerSlot = 4;    // units per workgroup slot the segment length aims at (where the batch has the tiles); measured: DESIGN.md 4.6
constexpr int kImdctMinSegment = 3;      // floor of S: 2 x (two tiles) - 1

inline long long imdct_tiles(long long frames, int tile_frames) { return frames <= 1 ? 0 : (frames + tile_frames - 1) / tile_frames; }
inline long long imdct_out_len(long long frames, int M) { return std::max<long long>((long long)M * (frames - 1) - 1, 0); }

// The batch's segment length in tiles.
inline long long imdct_segment_tiles(const int64_t* frames, int64_t n_clips, int tile_frames, long long slots, int per_slot = kImdctUnitsPerSlot) {
    long long total = 0;
    for (int64_t i = 0; i < n_clips; ++i) total += imdct_tiles(frames[i], tile_frames);
    const long long want = std::max<long long>(1, slots) * std::max(1, per_slot);
    return std::max<long long>(kImdctMinSegment, (total + want - 1) / want);
}

// The units of a batch, ordered for the deal.  The records carry the clip's index in `in_off` and nothing else of the clip: the caller, who
// knows pitches and offsets, fills the clip's fields in (imdct_fill_clip).
inline std::vector<ImdctUnit> imdct_cut_units(const int64_t* frames, int64_t n_clips, int tile_frames, long long slots, int per_slot = kImdctUnitsPerSlot) {
    const long long S = imdct_segment_tiles(frames, n_clips, tile_frames, slots, per_slot);
    std::vector<ImdctUnit> units;
    for (int64_t i = 0; i < n_clips; ++i) {
        const long long n = imdct_tiles(frames[i], tile_frames);
        if (n <= 0) continue;
        const long long k = (n + S - 1) / S, q = n / k, r = n % k;   // r segments of q + 1 tiles, then k - r of q
        long long a = 0;
        for (long long j = 0; j < k; ++j) {
            const long long len = q + (j < r ? 1 : 0);
            ImdctUnit u{};
            u.in_off = (long long)i;
            u.T = (int)frames[i], u.tiles = (int)n;
            u.tile_a = (int)a, u.tile_b = (int)(a + len);
            units.push_back(u);
            a += len;
        }
    }
    std::stable_sort(units.begin(), units.end(), [](const ImdctUnit& a, const ImdctUnit& b) { return a.tile_b - a.tile_a > b.tile_b - b.tile_a; });
    return units;
}

// The clip's fields of a unit that imdct_cut_units made: M rows of `pitch` floats at float `in_off`, the samples at float `out_off`.
inline void imdct_fill_clip(ImdctUnit& u, long long in_off, long long out_off, long long pitch, int M) {
    u.in_off = in_off, u.out_off = out_off, u.out_len = imdct_out_len(u.T, M), u.TP = (int)pitch;
}

// The deal: the table in launch order for `grid` workgroups -- workgroup wg walks positions wg, wg + grid, ... -- from the ordered units: rounds
// of `grid` neighbours, even rounds forwards, odd rounds backwards: the workgroup that took the longest unit of one round takes the shortest
// of the next.  Only the last round can be short; where a backward one leaves the first workgroups without a unit their positions hold a
// record without tiles (all zero: the kernel's tile loop and its gather pass over it), a forward one simply ends the table.
inline std::vector<ImdctUnit> imdct_deal_table(const std::vector<ImdctUnit>& units, long long grid) {
    const long long n = (long long)units.size();
    std::vector<ImdctUnit> table;
    if (n <= 0 || grid <= 0) return table;
    const long long rounds = (n + grid - 1) / grid;
    table.reserve((size_t)(rounds * grid));
    for (long long r = 0; r < rounds; ++r)
        for (long long wg = 0; wg < grid; ++wg) {
            const long long u = (r & 1) ? (r + 1) * grid - 1 - wg : r * grid + wg;
            if (u < n) table.push_back(units[(size_t)u]);
            else if (r & 1) table.push_back(ImdctUnit{});
        }
    return table;
}

}  // namespace zafx
