// zafx_maskfilter_pcm.hpp -- the sample arithmetic of the mask filter on 16-bit PCM (k_maskfilter_pcm, k_maskfilter_stereo_pcm,
// zafx_maskfilter_pcm.hip): how an int16 sample enters, how a float32 result leaves as int16, and the rest in integers.
//
//   * In.  Sample s enters as s / 32768 (zaf.py:1202, wavread's normalisation): exact in float32, and a power-of-two scale commutes with
//     every later rounding, so the float32 values inside the kernel are the float kernel's on x.astype(float32) / 32768, bit for bit.
//   * Out, int16.  The inverse of that normalisation.  With t = y * 32768 in float32 (exact unless it overflows to +-inf, which saturates):
//         NaN -> 0;   t >= 32767 (+inf too) -> 32767;   t <= -32768 (-inf too) -> -32768;   anything else -> rint(t), ties to even.
//     In NumPy: np.where(np.isnan(y), 0, np.clip(np.rint(y * np.float32(32768)), -32768, 32767)).astype(np.int16).
//   * Rest, int16.  rest = clamp(x - q(y), -32768, 32767) in integers: the subtraction of the y that was WRITTEN, so q(y) + rest == x to the
//     bit wherever the rest did not saturate (it can: x = -32768 under q(y) = 32767).
//
// Plain inline functions that also compile under -DZAFX_HOST_EMU with g++ (tests/host_emu/maskfilter_pcm_emu.cpp), as zafx_maskfilter.hpp does.
#pragma once
#include "zafx_maskfilter_stereo.hpp"

namespace zafx {

constexpr float kPcmUnit = 1.f / 32768.f;   // of one int16 step

// s / 32768 for an int16 sample s (any int of 24 bits or fewer converts exactly)
ZAFX_HD float pcm_sample(int s) { return (float)s * kPcmUnit; }

// q(y): the int16 sample of a float32 result, in an int
ZAFX_HD int pcm_quantise(float y) {
    const float t = y * 32768.f;
    if (t != t) return 0;   // NaN
    if (t >= 32767.f) return 32767;
    if (t <= -32768.f) return -32768;
    return (int)__builtin_rintf(t);   // ties to even (v_rndne_f32; the host runs in the default rounding mode)
}

// clamp(x - q, -32768, 32767) for two int16 values
ZAFX_HD int pcm_rest(int x, int q) {
    const int d = x - q;
    return d > 32767 ? 32767 : d < -32768 ? -32768 : d;
}

// One interleaved stereo sample frame (L, R) as the dword it is in memory (little-endian: L in the low half) ...
ZAFX_HD int pcm_pack(int l, int r) { return (int)(((unsigned)l & 0xffffu) | ((unsigned)r << 16)); }
// ... and back: the two channels sign-extended
ZAFX_HD int pcm_left(int d) { return (int)(short)(d & 0xffff); }
ZAFX_HD int pcm_right(int d) { return d >> 16; }

}  // namespace zafx
