// zafx_maskfilter_stereo.hpp -- the arithmetic between the two transforms of the stereo mask filter (k_maskfilter_stereo,
// zafx_maskfilter_stereo.hip).
//
// y[:, c] = istft(concat(m_c, m_c[-2:0:-1]) * stft(x[:, c], w, W/2), w, W/2)[0:N], c = L, R, for an interleaved stereo clip x (N, 2) and real
// masks of the caller's (zaf.py:176-198 with the caller's masks in place of the example's).  Both channels ride in ONE W-point complex
// transform Z = FFT(L + i R), as in k_center (zafx_center.hpp):
//     X_L[k] = (Z[k] + conj Z[W-k]) / 2,      X_R[k] = (Z[k] - conj Z[W-k]) / 2i.
//
//   * A mask per channel: C_L = m_0 X_L and C_R = m_1 X_R are Hermitian (the masks are real and mirrored), so the inverse transform of
//     C_L + i C_R returns the left channel in its real part and the right one in its imaginary part: center_pair's split and re-pack with
//     m_0, m_1 handed in instead of computed -- which is maskfilter_pair (zafx_maskfilter.hpp), on channels where that one has frames.
//   * One mask for both channels: C_L + i C_R = m (X_L + i X_R) = m Z.  No split: Z[k] and Z[W-k] are each scaled by m[k].
//
// Consequences of the packing: with a mask per channel the split rounds one channel's spectrum against the other's, so rounding error of the
// louder channel (about eps32 of ITS level) and a non-finite sample or mask value of one channel reach the other channel of the same frame --
// the two output blocks that frame contributes to --, never another frame pair or another clip.  The shared form never splits, but the two
// channels still share every butterfly of the two transforms: the same holds there.
//
// Not promised: that two equal per-channel masks give the shared form's bits (the split and re-pack round; the scaling of Z does not), nor
// that either channel has the bits k_maskfilter gives that channel as a mono clip (that kernel packs two FRAMES of one clip, this one two
// CHANNELS of one frame).  Both agree within the bound of the family (1e-5 of the level).
//
// Plain inline functions that also compile under -DZAFX_HOST_EMU with g++ (tests/host_emu/maskfilter_stereo_emu.cpp), as zafx_center.hpp does.
#pragma once
#include "zafx_maskfilter.hpp"

namespace zafx {

// frames of one tile, points per thread, windows: k_center's
constexpr int maskfilter_stereo_tile_frames(int log2w) { return center_tile_frames(log2w); }
constexpr int maskfilter_stereo_log2e(int log2w) { return center_log2e(log2w); }

// One pair (k, W-k) of the packed spectrum under a mask per channel: zk = Z[k], zn = Z[(W-k) mod W]; m0, m1: the masks of bin k of this frame
// for the left and the right channel.
//     ck = m_0 X_L[k] + i m_1 X_R[k],   cn = conj(m_0 X_L[k]) + i conj(m_1 X_R[k]).
// k = 0 and k = W/2 pair with themselves (zn = zk): then ck == cn.
ZAFX_HD void maskfilter_stereo_pair(float2 zk, float2 zn, float m0, float m1, float2& ck, float2& cn) { maskfilter_pair(zk, zn, m0, m1, ck, cn); }

// The same pair under ONE mask m for both channels: ck = m Z[k], cn = m Z[W-k].  (Both are read before either is written back: at k = 0 and
// k = W/2 they are the same element, and ck == cn.)
ZAFX_HD void maskfilter_stereo_pair_shared(float2 zk, float2 zn, float m, float2& ck, float2& cn) {
    ck = cscale(zk, m);
    cn = cscale(zn, m);
}

}  // namespace zafx
