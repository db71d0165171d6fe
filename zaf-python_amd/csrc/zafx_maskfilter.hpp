// zafx_maskfilter.hpp -- the arithmetic between the two transforms of the mask filter (k_maskfilter, zafx_maskfilter.hip).
//
// y = istft(concat(m, m[-2:0:-1]) * stft(x, w, W/2), w, W/2)[0:N] for a mono clip x and a real mask m of the caller's, (W/2 + 1, T): what
// zaf.istft's docstring does with its own masks (zaf.py:185-195).  Two neighbouring frames of the SAME clip ride in one W-point complex
// transform, Z = FFT(a + i b) with a = w * frame 2j, b = w * frame 2j+1:
//     A[k] = (Z[k] + conj Z[W-k]) / 2,      B[k] = (Z[k] - conj Z[W-k]) / 2i,
// and the masked spectra m[k, 2j] A and m[k, 2j+1] B are Hermitian (the mask is real and mirrored), so the inverse transform of
// m_a A + i m_b B returns masked frame 2j in its real part and masked frame 2j+1 in its imaginary part.  That is center_pair
// (zafx_center.hpp) with the two masks handed in instead of computed.
//
// Consequence of the packing: the split rounds one frame's spectrum against the other's, so rounding error -- and a non-finite value -- of
// frame 2j+1 reaches frame 2j and the reverse: H samples further than in the unpacked computation, never another clip.
//
// Plain inline functions that also compile under -DZAFX_HOST_EMU with g++ (tests/host_emu/maskfilter_emu.cpp), as zafx_center.hpp does.
#pragma once
#include "zafx_center.hpp"

namespace zafx {

// packed transforms of one tile of k_maskfilter (a tile is twice as many frames), points per thread, windows: k_center's
constexpr int maskfilter_tile_transforms(int log2w) { return center_tile_frames(log2w); }
constexpr int maskfilter_log2e(int log2w) { return center_log2e(log2w); }
constexpr bool maskfilter_supported(int log2w) { return center_supported(log2w); }

// One pair (k, W-k) of the packed spectrum: zk = Z[k], zn = Z[(W-k) mod W]; ma, mb: the mask of bin k in frame 2j and in frame 2j+1.
//     ck = m_a A[k] + i m_b B[k],   cn = conj(m_a A[k]) + i conj(m_b B[k]).
// k = 0 and k = W/2 pair with themselves (zn = zk): then ck == cn.
ZAFX_HD void maskfilter_pair(float2 zk, float2 zn, float ma, float mb, float2& ck, float2& cn) {
    const float2 a2 = cadd_conj(zk, zn);            // 2 A[k]
    const float2 b2 = mul_mi(csub_conj(zk, zn));    // 2 B[k]
    const float2 ca = cscale(a2, 0.5f * ma), cb = cscale(b2, 0.5f * mb);
    ck = make_float2(ca.x - cb.y, ca.y + cb.x);
    cn = make_float2(ca.x + cb.y, cb.x - ca.y);
}

// The same pair under a COMPLEX mask M of the caller's, extended to its Hermitian mirror (M[W-k] = conj M[k]): ma, mb = M[k, 2j], M[k, 2j+1].
// M_a A and M_b B are Hermitian again, so the re-pack is the one above with two complex products in place of the two scalings:
//     ck = M_a A[k] + i M_b B[k],   cn = conj(M_a A[k]) + i conj(M_b B[k]).
// k = 0 and k = W/2 pair with themselves, and their mirror is themselves: only Re M acts there (zaf.istft keeps the real part, zaf.py:223).
// The CALLER hands those two bins' masks in with .y = 0 -- the value it was given is discarded, not multiplied by zero, so it may be
// anything, NaN included --; then A, B and both products are real and ck == cn.
// Not the bits of maskfilter_pair at Im M = 0: under -ffp-contract=fast the products contract differently.
ZAFX_HD void maskfilter_pair_c(float2 zk, float2 zn, float2 ma, float2 mb, float2& ck, float2& cn) {
    const float2 a2 = cadd_conj(zk, zn);            // 2 A[k]
    const float2 b2 = mul_mi(csub_conj(zk, zn));    // 2 B[k]
    const float2 ca = cmul(a2, cscale(ma, 0.5f)), cb = cmul(b2, cscale(mb, 0.5f));
    ck = make_float2(ca.x - cb.y, ca.y + cb.x);
    cn = make_float2(ca.x + cb.y, cb.x - ca.y);
}

// frames of a clip of n samples at hop H = W/2 (zaf.py:99-109): ceil(n / H) + 1
constexpr long long maskfilter_frames(long long n_samples, int W) { return (n_samples + W / 2 - 1) / (W / 2) + 1; }

}  // namespace zafx
