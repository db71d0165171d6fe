// zafx_units.hpp -- a ragged batch cut into the units a RAGGED kernel form walks: k_center's (zafx_center.hip, zafx_execute_center_ragged),
// k_maskfilter's (zafx_maskfilter.hip, zafx_execute_masked_ragged) and k_maskfilter_stems' (zafx_maskfilter_stems.hip,
// zafx_execute_masked_stems_ragged: the same records and cut, the slots of the stems' LDS size), k_imdct's (zafx_mdct.hip, zafx_execute_imdct_ragged) and k_istft_ft16's
// (zafx_stft.hip, zafx_execute_istft_ragged).  Beside it the cuts of equal-length batches: center_equal_segments / maskfilter_equal_segments for
// k_center, k_maskfilter and k_maskfilter_stems (their launchers call them), carry_segments for the carry kernels.
//
// A clip is a run of pieces: blocks of H = W / 2 sample frames for k_center, pairs of such blocks (one packed transform) for k_maskfilter, tiles
// of `tile_frames` frames for k_imdct and k_istft_ft16.  One unit = pieces [a, b) of one clip.  A unit that does not start its clip pays a fixed
// entry cost -- k_center a halo frame, k_imdct and k_istft_ft16 the tile in front of it in carry-only mode; k_maskfilter's pays at its END, the
// halo transform behind an even last block -- and for that gives the same bits wherever it starts.
//
// The rule (cut_segments): one segment length S in pieces for the whole batch,
//     S = max(floor, ceil(total pieces / (per_slot x workgroup slots)));
// a clip of at most S pieces is one unit, a longer one of n pieces is cut into k = ceil(n / S) near-equal segments: with q = n / k and
// r = n % k, r segments of q + 1 pieces, then k - r of q.  A clip without pieces gives no unit.  The units are ordered by descending size
// (stable: ties keep clip order, then a) and dealt in rounds of `grid` neighbours in that order, forwards and backwards in turn, so the
// workgroups' sums stay within about one unit of each other.  A fixed deal: nothing is claimed at run time.
//
// The floor.  Every segment of a cut clip is to keep at least m pieces -- what amortises the entry cost -- and none may exceed S.  The second
// holds for any S: k >= n / S, so n / k <= S and ceil(n / k) <= S.  The first, q >= m, is n >= m k; with k <= (n + S - 1) / S it follows from
// m (S - 1) <= n (S - m), and a cut clip has n >= S + 1, so from m (S - 1) <= (S + 1) (S - m), which is S >= 2 m - 1.  S = 2 m - 2 is too
// small: a clip of 2 m - 1 pieces would be cut into m and m - 1.  So floor = 2 m - 1:
//     k_center: m = 2 F - 1 blocks, the two tiles of F frames that are the floor of the equal-length launch: floor = 2 (2 F - 1) - 1 = 4 F - 3;
//     k_maskfilter: m = 2 F - 1 block pairs, with the halo transform two tiles of F transforms:             floor = 2 (2 F - 1) - 1 = 4 F - 3;
//     k_imdct:  m = 2 tiles:                                                                               floor = 2 x 2 - 1 = 3;
//     k_istft_ft16: the carry-only tile transforms at most `halo` < 16 of its 16 frames, m = 2 tiles:      floor = 2 x 2 - 1 = 3.
//
// Plain C++17, no HIP: hipcc compiles it into the library, g++ into tests/host_emu/{center,maskfilter,tile}_units_emu.cpp, equal_segments_emu.cpp, carry_segments_emu.cpp and the
// host layer's sanitizer build.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace zafx {

struct Segment { int64_t clip; long long a, b; };   // pieces [a, b) of a clip

// The batch's segment length in pieces; counts[i]: the pieces of clip i.
inline long long segment_length(const long long* counts, int64_t n, long long floor, long long slots, int per_slot) {
    long long total = 0;
    for (int64_t i = 0; i < n; ++i) total += counts[i];
    const long long want = std::max<long long>(1, slots) * std::max(1, per_slot);
    return std::max(floor, (total + want - 1) / want);
}

// The batch's segments, ordered for the deal.
inline std::vector<Segment> cut_segments(const long long* counts, int64_t n, long long floor, long long slots, int per_slot) {
    const long long S = segment_length(counts, n, floor, slots, per_slot);
    std::vector<Segment> segs;
    for (int64_t i = 0; i < n; ++i) {
        if (counts[i] <= 0) continue;
        const long long k = (counts[i] + S - 1) / S, q = counts[i] / k, r = counts[i] % k;
        long long a = 0;
        for (long long j = 0; j < k; ++j) {
            const long long len = q + (j < r ? 1 : 0);
            segs.push_back({i, a, a + len});
            a += len;
        }
    }
    std::stable_sort(segs.begin(), segs.end(), [](const Segment& x, const Segment& y) { return x.b - x.a > y.b - y.a; });
    return segs;
}

// The deal: the table in launch order for `grid` workgroups -- workgroup wg walks positions wg, wg + grid, ... -- from the ordered units: rounds
// of `grid` neighbours, even rounds forwards, odd rounds backwards: the workgroup that took the longest unit of one round takes the shortest
// of the next.  Only the last round can be short; where a backward one leaves the first workgroups without a unit their positions hold a
// value-initialised record (no pieces: the kernel passes over it), a forward one simply ends the table.
template <class Unit>
std::vector<Unit> deal_table(const std::vector<Unit>& units, long long grid) {
    const long long n = (long long)units.size();
    std::vector<Unit> table;
    if (n <= 0 || grid <= 0) return table;
    const long long rounds = (n + grid - 1) / grid;
    table.reserve((size_t)(rounds * grid));
    for (long long r = 0; r < rounds; ++r)
        for (long long wg = 0; wg < grid; ++wg) {
            const long long u = (r & 1) ? (r + 1) * grid - 1 - wg : r * grid + wg;
            if (u < n) table.push_back(units[(size_t)u]);
            else if (r & 1) table.push_back(Unit{});
        }
    return table;
}

template <class Count>
std::vector<long long> piece_counts(const int64_t* sizes, int64_t n, Count count) {
    std::vector<long long> counts((size_t)std::max<int64_t>(n, 0));
    for (size_t i = 0; i < counts.size(); ++i) counts[i] = count((long long)sizes[i]);
    return counts;
}

// ---- k_center: blocks.  One record of the device table.  Offsets and lengths in sample frames (one sample frame = 8 bytes: L, R).  The kernel deals the rounds itself.
struct CenterUnit {
    long long in_off, n_samples, out_off;   // the unit's CLIP: its first sample frame in the input, its length, its first sample frame in the output
    int b0, b1;                             // the unit: blocks [b0, b1) of that clip
};
static_assert(sizeof(CenterUnit) == 32 && alignof(CenterUnit) == 8, "CenterUnit: the layout the host writes");

constexpr int kCenterUnitsPerSlot = 12;   // units per workgroup slot the segment length aims at (where the batch has the blocks); measured: DESIGN.md 4.7

inline long long center_blocks(long long n_samples, int W) { return (n_samples + W / 2 - 1) / (W / 2); }

inline long long center_segment_blocks(const int64_t* lengths, int64_t n_clips, int W, int F, long long slots, int per_slot = kCenterUnitsPerSlot) {
    const auto counts = piece_counts(lengths, n_clips, [W](long long n) { return center_blocks(n, W); });
    return segment_length(counts.data(), n_clips, 4LL * F - 3, slots, per_slot);
}

// in_offsets / out_offsets: null = 0 for every clip.
inline std::vector<CenterUnit> center_cut_units(const int64_t* lengths, const int64_t* in_offsets, const int64_t* out_offsets, int64_t n_clips, int W,
                                                int F, long long slots, int per_slot = kCenterUnitsPerSlot) {
    const auto counts = piece_counts(lengths, n_clips, [W](long long n) { return center_blocks(n, W); });
    std::vector<CenterUnit> units;
    for (const Segment& s : cut_segments(counts.data(), n_clips, 4LL * F - 3, slots, per_slot))
        units.push_back({in_offsets ? (long long)in_offsets[s.clip] : 0LL, (long long)lengths[s.clip], out_offsets ? (long long)out_offsets[s.clip] : 0LL,
                         (int)s.a, (int)s.b});
    return units;
}

// ---- k_maskfilter: pairs of blocks.  One record of the device table.  Offsets and lengths in float32 elements.  The kernel deals the rounds itself.
// The piece is one packed transform's two blocks: a clip of n_blocks = ceil(n / H) blocks has ceil(n_blocks / 2) pieces, and the segment of
// pieces [a, b) is blocks [2 a, min(n_blocks, 2 b)) -- every segment starts on an even block, which the kernel requires, and all but a clip's
// last end on one (those run one transform more, the halo).  k_maskfilter_stems reads the same record: mask_off is the first of the clip's S
// compact TF masks, which lie back to back, out_off the first of its S (+ 1 with the rest) output blocks of n_samples, mask_pitch is not used.  m = 2 F - 1 pieces: with the halo two full tiles of F transforms, the floor of
// the equal-length launch; floor of S = 2 m - 1 = 4 F - 3, as for k_center.
struct MaskfilterUnit {
    long long in_off, n_samples, out_off, mask_off;   // the unit's CLIP: its first sample in the input, its length, its first sample in the output, the first element of its mask
    int b0, b1;                                       // the unit: blocks [b0, b1) of that clip, b0 even
    int mask_pitch, pad_;                             // elements between the rows of the clip's mask (ZAFX_LAYOUT_FT; TF masks are compact: not used)
};
static_assert(sizeof(MaskfilterUnit) == 48 && alignof(MaskfilterUnit) == 8, "MaskfilterUnit: the layout the host writes");

constexpr int kMaskfilterUnitsPerSlot = 8;   // units per workgroup slot the segment length aims at (where the batch has the pieces); measured: DESIGN.md 4.12 (k_center's 12 costs 2 %)

inline long long maskfilter_pieces(long long n_samples, int W) { return (center_blocks(n_samples, W) + 1) / 2; }

// in_offsets / out_offsets / mask_offsets / mask_pitches: null = 0 for every clip.
inline std::vector<MaskfilterUnit> maskfilter_cut_units(const int64_t* lengths, const int64_t* in_offsets, const int64_t* out_offsets, const int64_t* mask_offsets,
                                                        const int64_t* mask_pitches, int64_t n_clips, int W, int F, long long slots,
                                                        int per_slot = kMaskfilterUnitsPerSlot) {
    const auto counts = piece_counts(lengths, n_clips, [W](long long n) { return maskfilter_pieces(n, W); });
    std::vector<MaskfilterUnit> units;
    for (const Segment& s : cut_segments(counts.data(), n_clips, 4LL * F - 3, slots, per_slot)) {
        const long long n_blocks = center_blocks((long long)lengths[s.clip], W);
        units.push_back({in_offsets ? (long long)in_offsets[s.clip] : 0LL, (long long)lengths[s.clip], out_offsets ? (long long)out_offsets[s.clip] : 0LL,
                         mask_offsets ? (long long)mask_offsets[s.clip] : 0LL, (int)(2 * s.a), (int)std::min(n_blocks, 2 * s.b),
                         mask_pitches ? (int)mask_pitches[s.clip] : 0, 0});
    }
    return units;
}

// ---- k_maskfilter_stereo (zafx_maskfilter_stereo.hip, zafx_execute_masked_stereo_ragged): k_center's pieces and rule -- blocks, the halo frame
// in front of a unit that does not start its clip, floor 4 F - 3 -- in MaskfilterUnit records, which carry what k_center's lack: mask_off, the
// first float32 element of the clip's mask(s).  Offsets and lengths of samples in sample frames; b0 is any block, mask_pitch is not used.
inline std::vector<MaskfilterUnit> maskfilter_stereo_cut_units(const int64_t* lengths, const int64_t* in_offsets, const int64_t* out_offsets, const int64_t* mask_offsets,
                                                               int64_t n_clips, int W, int F, long long slots, int per_slot = kCenterUnitsPerSlot) {
    const auto counts = piece_counts(lengths, n_clips, [W](long long n) { return center_blocks(n, W); });
    std::vector<MaskfilterUnit> units;
    for (const Segment& s : cut_segments(counts.data(), n_clips, 4LL * F - 3, slots, per_slot))
        units.push_back({in_offsets ? (long long)in_offsets[s.clip] : 0LL, (long long)lengths[s.clip], out_offsets ? (long long)out_offsets[s.clip] : 0LL,
                         mask_offsets ? (long long)mask_offsets[s.clip] : 0LL, (int)s.a, (int)s.b, 0, 0});
    return units;
}

// ---- k_center, k_maskfilter and k_maskfilter_stems on equal-length batches: every clip has the same n_blocks > 0, cut into `segs` segments of
// `seg_blocks` blocks (the last one shorter, never empty); unit u = clip * segs + seg.  Whole clips when there are enough of them to load
// every workgroup slot (n_clips >= slots); otherwise about two units per slot.
struct EqualSegments { int64_t seg_blocks; long long segs; };

// k_center: never below two tiles (2 F - 1 blocks) a segment -- each pays one halo frame.
inline EqualSegments center_equal_segments(int64_t n_blocks, int64_t n_clips, int F, long long slots) {
    long long segs = std::max<long long>(1, (2 * slots + n_clips - 1) / n_clips);
    if (n_clips >= slots) segs = 1;
    segs = std::min<long long>(segs, std::max<long long>(1, n_blocks / (2 * F - 1)));
    const int64_t seg_blocks = (n_blocks + segs - 1) / segs;
    return {seg_blocks, (long long)((n_blocks + seg_blocks - 1) / seg_blocks)};
}

// k_maskfilter, k_maskfilter_stems: seg_blocks is even (a segment starts on a transform of its own), and a cut clip goes into runs of
// 2 F m - 2 blocks, m >= 2: such a run ends on an even block, and its F m transforms -- the halo included -- fill m tiles exactly.
inline EqualSegments maskfilter_equal_segments(int64_t n_blocks, int64_t n_clips, int F, long long slots) {
    const long long want = n_clips >= slots ? 1 : std::max<long long>(1, (2 * slots + n_clips - 1) / n_clips);
    int64_t seg_blocks = (n_blocks + 1) & ~(int64_t)1;
    if (want > 1) {
        const int64_t ideal = (n_blocks + want - 1) / want;
        const int64_t m = std::max<int64_t>(2, (ideal + 2 + 2 * F - 1) / (2 * F));
        seg_blocks = std::min<int64_t>(seg_blocks, 2 * (int64_t)F * m - 2);
    }
    return {seg_blocks, (long long)((n_blocks + seg_blocks - 1) / seg_blocks)};
}

// ---- k_imdct and k_istft_ft16: tiles.  One record of the device table, the same for both kernels.  The host deals the rounds (deal_table).
struct TileUnit {
    long long in_off, out_off, out_len;   // the unit's CLIP: its block in the input array (k_imdct: floats; k_istft_ft16: complex64 elements), its first sample in the output and its samples (floats)
    int T, TP, tiles;                     // ... its frames, the pitch of its rows in frames, its tiles
    int tile_a, tile_b, pad_;             // the unit: tiles [tile_a, tile_b) of that clip
};
static_assert(sizeof(TileUnit) == 48 && alignof(TileUnit) == 8, "TileUnit: the layout the host writes");

// counts[i]: the tiles of clip i.  The records carry the clip's index in `in_off` and nothing else of the clip: the caller, who knows the plan's
// pitches, fills the rest in (tile_fill_clip).
inline std::vector<TileUnit> tile_cut_units(const std::vector<long long>& counts, const int64_t* frames, int64_t n_clips, long long floor, long long slots,
                                            int per_slot) {
    std::vector<TileUnit> units;
    for (const Segment& s : cut_segments(counts.data(), n_clips, floor, slots, per_slot)) {
        TileUnit u{};
        u.in_off = (long long)s.clip;
        u.T = (int)frames[s.clip], u.tiles = (int)counts[(size_t)s.clip];
        u.tile_a = (int)s.a, u.tile_b = (int)s.b;
        units.push_back(u);
    }
    return units;
}

// ... rows of `pitch` elements at element `in_off`, the `out_len` samples at float `out_off`.
inline void tile_fill_clip(TileUnit& u, long long in_off, long long out_off, long long pitch, long long out_len) {
    u.in_off = in_off, u.out_off = out_off, u.out_len = out_len, u.TP = (int)pitch;
}

// ---- k_imdct: tiles of 32 frames at W = 512, 1024, 2048.
constexpr int kImdctUnitsPerSlot = 4;    // units per workgroup slot the segment length aims at (where the batch has the tiles); measured: DESIGN.md 4.6
constexpr int kImdctMinSegment = 3;      // floor of S

// A clip whose output is empty (T <= 1: the reference returns y[M : -M-1], max(M (T - 1) - 1, 0) samples) has no tiles.
inline long long imdct_tiles(long long frames, int tile_frames) { return frames <= 1 ? 0 : (frames + tile_frames - 1) / tile_frames; }
inline long long imdct_out_len(long long frames, int M) { return std::max<long long>((long long)M * (frames - 1) - 1, 0); }

inline std::vector<long long> imdct_tile_counts(const int64_t* frames, int64_t n_clips, int tile_frames) {
    return piece_counts(frames, n_clips, [tile_frames](long long t) { return imdct_tiles(t, tile_frames); });
}
inline long long imdct_segment_tiles(const int64_t* frames, int64_t n_clips, int tile_frames, long long slots, int per_slot = kImdctUnitsPerSlot) {
    return segment_length(imdct_tile_counts(frames, n_clips, tile_frames).data(), n_clips, kImdctMinSegment, slots, per_slot);
}
inline std::vector<TileUnit> imdct_cut_units(const int64_t* frames, int64_t n_clips, int tile_frames, long long slots, int per_slot = kImdctUnitsPerSlot) {
    return tile_cut_units(imdct_tile_counts(frames, n_clips, tile_frames), frames, n_clips, kImdctMinSegment, slots, per_slot);
}

// ---- k_istft_ft16: tiles of 16 frames.
constexpr int kIstftUnitsPerSlot = 4;    // units per workgroup slot the segment length aims at (where the batch has the tiles): k_imdct's measured value, whose units pay the same entry cost; the ISTFT's own sweep (tools/ragged_rates.py --istft-k) has not chosen it: DESIGN.md 4.6
constexpr int kIstftMinSegment = 3;      // floor of S

// zaf.py istft: T frames at hop H overlap-add to (T - 1) H + W samples, W - H are trimmed at either end.  A spectrum whose output is empty has
// no tiles and gives no unit.
inline long long istft_out_len(long long frames, int W, int H) { return std::max<long long>(frames * H - (W - H), 0); }
inline long long istft_tiles(long long frames, int tile_frames) { return frames <= 0 ? 0 : (frames + tile_frames - 1) / tile_frames; }

inline std::vector<long long> istft_tile_counts(const int64_t* frames, int64_t n_clips, int W, int H, int tile_frames) {
    return piece_counts(frames, n_clips, [=](long long t) { return istft_out_len(t, W, H) > 0 ? istft_tiles(t, tile_frames) : 0LL; });
}
inline long long istft_segment_tiles(const int64_t* frames, int64_t n_clips, int W, int H, int tile_frames, long long slots, int per_slot = kIstftUnitsPerSlot) {
    return segment_length(istft_tile_counts(frames, n_clips, W, H, tile_frames).data(), n_clips, kIstftMinSegment, slots, per_slot);
}
inline std::vector<TileUnit> istft_cut_units(const int64_t* frames, int64_t n_clips, int W, int H, int tile_frames, long long slots,
                                             int per_slot = kIstftUnitsPerSlot) {
    return tile_cut_units(istft_tile_counts(frames, n_clips, W, H, tile_frames), frames, n_clips, kIstftMinSegment, slots, per_slot);
}

// ---- the carry kernels of equal-length batches (k_stft_ft16c, k_istft_ft16 and its band forms, k_imdct, k_mdct_ft32's carry forms, the float64
// inverses): every clip has the same `tiles`.  Cut every clip's tiles into `segs` segments so that a persistent grid of `grid` workgroups is
// evenly loaded: whole clips when there are enough of them, otherwise shorter segments (each pays one carry-only tile, counted as half a
// tile).  The cost is rounds x (tiles of a segment + 0.5 for segs > 1); of the cuts without an empty segment the first of the cheapest wins.
inline int carry_segments(long long n_clips, int tiles, long long grid) {
    int best = 1;
    double best_cost = 1e300;
    for (int segs = 1; segs <= tiles; ++segs) {
        const int seg_tiles = (tiles + segs - 1) / segs;
        if (segs > 1 && (segs - 1) * seg_tiles >= tiles) continue;   // would leave an empty segment
        const long long rounds = (n_clips * segs + grid - 1) / grid;
        const double cost = (double)rounds * (seg_tiles + (segs > 1 ? 0.5 : 0.0));
        if (cost < best_cost - 1e-9) best_cost = cost, best = segs;
    }
    return best;
}

}  // namespace zafx
