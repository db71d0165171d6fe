// zafx_center.hpp -- the arithmetic between the two transforms of the center / sides extraction (k_center, zafx_center.hip).
//
// The example in zaf.istft's docstring (zaf.py:155-198): STFT of the left and the right channel, the two time-frequency masks
// min(|L|, |R|) / |L| and min(|L|, |R|) / |R| on rows 0 .. W/2 mirrored onto the upper rows, ISTFT of the masked spectra,
// sides = input - center.  Both channels ride in ONE W-point complex transform Z = FFT(L + i R):
//     X_L[k] = (Z[k] + conj Z[W-k]) / 2,      X_R[k] = (Z[k] - conj Z[W-k]) / 2i,
// and the masked spectra C_L = m_0 X_L, C_R = m_1 X_R are Hermitian (the masks are real and mirrored), so the inverse transform of
// C_L + i C_R returns the center's left channel in its real part and the right channel in its imaginary part.
//
// Mask form -- the one deliberate departure from the reference: m_0 = (b < a) ? b / a : 1, m_1 = (a < b) ? a / b : 1 with a = |X_L|,
// b = |X_R|.  That equals np.minimum(a, b) / a wherever the latter is finite; where the reference divides 0 by 0 (an exactly
// silent bin, which it turns into a whole frame of NaNs) the masked bin is 0, the limit value.
//
// Plain inline functions that also compile under -DZAFX_HOST_EMU with g++ (tests/host_emu/center_emu.cpp), as zafx_fft.hpp does.
#pragma once
#include "zafx_fft.hpp"

namespace zafx {

// frames of one tile of k_center: a workgroup transforms that many side by side.  4 at W = 2048: its 512 threads may then hold the 160 - 180
// registers the 16-point-per-lane transform with its tables in flight takes (8 frames = 1024 threads leave 128: 200 - 270 bytes of scratch)
constexpr int center_tile_frames(int log2w) { return log2w >= 11 ? 4 : 8; }
// points per thread: W / 64, so that 64 lanes own one frame, up to W = 1024; 16 at W = 2048 (two wavefronts per frame)
constexpr int center_log2e(int log2w) { return log2w >= 11 ? 4 : log2w - 6; }
constexpr bool center_supported(int log2w) { return log2w >= 8 && log2w <= 11; }

// lo / hi for 0 <= lo < hi.  The device form is one v_rcp_f32 (1 ulp) and a multiply; a denominator below the smallest normal
// number (|X| < 1e-19) is raised to it: v_rcp_f32 takes a denormal for zero.
ZAFX_HD float center_ratio(float lo, float hi) {
    const float den = hi < 1.17549435e-38f ? 1.17549435e-38f : hi;
#if defined(__HIP_DEVICE_COMPILE__)
    return lo * __builtin_amdgcn_rcpf(den);
#else
    return lo / den;
#endif
}
ZAFX_HD float center_sqrt(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sqrtf(v);
#else
    return std::sqrt(v);
#endif
}

// The two masks of one bin from the squared magnitudes pa = |X_L|^2, pb = |X_R|^2 (any common factor cancels): only one of
// them differs from 1, and it is sqrt(min / max) -- one reciprocal and one square root per bin.
ZAFX_HD void center_masks(float pa, float pb, float& m0, float& m1) {
    const bool l_big = pb < pa, r_big = pa < pb;
    const float r = center_sqrt(center_ratio(l_big ? pb : pa, l_big ? pa : pb));
    m0 = l_big ? r : 1.f;
    m1 = r_big ? r : 1.f;
}

// One pair (k, W-k) of the packed spectrum: zk = Z[k], zn = Z[(W-k) mod W].  Split, mask, re-pack:
//     ck = C_L[k] + i C_R[k],   cn = C_L[W-k] + i C_R[W-k] = conj C_L[k] + i conj C_R[k].
// k = 0 and k = W/2 pair with themselves (zn = zk): then ck == cn.
ZAFX_HD void center_pair(float2 zk, float2 zn, float2& ck, float2& cn) {
    const float2 l2 = cadd_conj(zk, zn);            // 2 X_L[k]
    const float2 r2 = mul_mi(csub_conj(zk, zn));    // 2 X_R[k]
    float m0, m1;
    center_masks(l2.x * l2.x + l2.y * l2.y, r2.x * r2.x + r2.y * r2.y, m0, m1);
    const float2 cl = cscale(l2, 0.5f * m0), cr = cscale(r2, 0.5f * m1);
    ck = make_float2(cl.x - cr.y, cl.y + cr.x);
    cn = make_float2(cl.x + cr.y, cr.x - cl.y);
}

// The inverse transform runs on the forward core: IFFT(X) = swap(FFT(swap X)) / W with swap(a + i b) = b + i a.
ZAFX_HD float2 center_swap(float2 a) { return make_float2(a.y, a.x); }

}  // namespace zafx
