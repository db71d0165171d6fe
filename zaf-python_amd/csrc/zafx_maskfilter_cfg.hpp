// zafx_maskfilter_cfg.hpp -- the launch geometry and LDS layout of k_maskfilter (zafx_maskfilter.hip), shared with k_maskfilter_stems
// (zafx_maskfilter_stems.hip), which runs on the same frames, carry and tables, and with k_maskfilter_pcm (zafx_maskfilter_pcm.hip); and those
// of k_maskfilter_stereo (zafx_maskfilter_stereo.hip), shared with k_maskfilter_stereo_pcm.
#pragma once
#include "zafx_maskfilter_stereo.hpp"
#include "zafx_internal.hpp"

namespace zafx {

template <int LOG2W, bool TF>
struct MaskfilterCfg {
    static constexpr int LOG2E = maskfilter_log2e(LOG2W);
    using C = FftCfg<LOG2W, LOG2E>;
    static constexpr int W = 1 << LOG2W, H = W / 2, E = C::E, P = C::P, F = maskfilter_tile_transforms(LOG2W), NT = P * F;
    static_assert(P == 64 || P == 128, "k_maskfilter: one or two wavefronts per transform");
    // LDS (float2 slots): F padded frames | the carry (imaginary second half of the tile's last transform, H floats) | the pass tables
    // ZAFX_LAYOUT_FT: | the mask stage: FS frames of every row, rows SP floats apart (FS = two tiles; 32 frames are one 128-byte line of a row)
    static constexpr int FS = LOG2W >= 11 ? 16 : 32, SP = FS + 2;
    static_assert(FS == 4 * F, "k_maskfilter: a mask stage is two tiles");
    static constexpr int OFF_CARRY = F * C::PITCH, OFF_TW = OFF_CARRY + H / 2, OFF_STAGE = OFF_TW + C::TW;
    static constexpr int SLOTS = OFF_STAGE + (TF ? 0 : ((H + 1) * SP + 1) / 2);
    static constexpr size_t SMEM = (size_t)SLOTS * 8;
    static_assert(SMEM <= (size_t)kMaxLdsBytes, "k_maskfilter: frames + carry + tables exceed LDS");
};

// k_maskfilter_stereo: k_center's geometry and LDS layout (CenterCfg, zafx_center.hip), restated: that translation unit stays as it is.
template <int LOG2W>
struct MaskfilterStereoCfg {
    static constexpr int LOG2E = maskfilter_stereo_log2e(LOG2W);
    using C = FftCfg<LOG2W, LOG2E>;
    static constexpr int W = 1 << LOG2W, H = W / 2, E = C::E, P = C::P, F = maskfilter_stereo_tile_frames(LOG2W), NT = P * F;
    static_assert(P == 64 || P == 128, "k_maskfilter_stereo: one or two wavefronts per frame");
    // LDS (float2 slots): F padded frames | the carry (second half of the tile's last frame, H points) | the pass tables
    static constexpr int OFF_CARRY = F * C::PITCH, OFF_TW = OFF_CARRY + H, SLOTS = OFF_TW + C::TW;
    static constexpr size_t SMEM = (size_t)SLOTS * 8;
    static_assert(SMEM <= (size_t)kMaxLdsBytes, "k_maskfilter_stereo: frames + carry + tables exceed LDS");
};

}  // namespace zafx
