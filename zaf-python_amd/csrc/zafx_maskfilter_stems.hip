// zafx_maskfilter_stems.hip -- k_maskfilter_stems: the mask filter with S masks per clip (the stems of a source separation): one STFT, S masks,
// S ISTFTs of mono clips in one kernel (zafx_execute_masked_stems; clips of different lengths: its RAGGED form, zafx_execute_masked_stems_ragged).
// A translation unit of its own: k_maskfilter's instantiations (zafx_maskfilter.hip) keep their registers to the last one.
#include <algorithm>

#include "zafx_maskfilter_cfg.hpp"
#include "zafx_units.hpp"
#include "zafx_overlap_walk.hpp"

namespace zafx {

// ---------------------------------------------------------------------------------
// stems (zafx_execute_masked_stems): S masks over one forward transform, S inverse transforms, in one kernel
// ---------------------------------------------------------------------------------
// k_maskfilter's plan -- segments, tiles, the samples' descriptor, the pair arithmetic, the inverse on the forward core, the two-term overlap-add,
// the gain -- with a loop over the stems between the forward transform and the tile's end (DESIGN.md 4.12 "Stems"):
//   * The inverse runs in place in the LDS frame and destroys the spectrum, so a lane takes the spectrum of its pairs (k, W - k) into registers
//     behind the forward transform (2 E floats, lane 0 bin H as well) and forms every stem's masked pairs from there.  A lane is the only
//     reader and writer of its pairs' slots, so no barrier stands between the forward transform and the first stem's pairs.
//   * One carry per stem: carry 0 where k_maskfilter has its one, carries 1 .. S - 1 behind the pass tables (stems_smem).
//   * Masks: (B, S, T, W/2 + 1), ZAFX_LAYOUT_TF, one descriptor per (clip, stem).  Stem 0's values are loaded in front of the forward transform as
//     k_maskfilter's are; stem s + 1's are loaded into the same registers as soon as stem s's pairs are formed, under stem s's inverse.
//   * Output (B, S, N); REST: (B, S + 1, N), block S = ((x - y_0) - y_1) - ... - y_{S-1}, subtracted in place from the samples as loaded.
// Stem s of a clip has the bits k_maskfilter gives that clip with mask s alone: every value passes through the same inline functions in the same
// order, and no stem's arithmetic reads another stem's values.
template <int LOG2W>
constexpr size_t maskfilter_stems_smem(int n_stems) {
    return MaskfilterCfg<LOG2W, true>::SMEM + (size_t)(n_stems - 1) * MaskfilterCfg<LOG2W, true>::H * 4;
}

// unit u = clip * n_segs + seg as in k_maskfilter; stem s of a clip: mask at (clip * n_stems + s) * mask_clip, output at (clip * blocks_out + s) * n_samples,
// blocks_out = n_stems + REST
// RAGGED (zafx_execute_masked_stems_ragged): clips of different lengths, as k_maskfilter's RAGGED form has them.  `n_samples` carries the table
// of unit records (the equal-length instantiations keep their kernel arguments byte for byte), unit u is record u -- its clip's samples at
// x + in_off, n_samples of them, its S masks back to back at mask + mask_off, each (n_blocks + 1) (H + 1) elements with a descriptor of its
// own, its S (+ REST) output blocks of n_samples back to back at out + out_off --, and mask_clip / n_blocks / seg_blocks / n_segs are not used.
template <bool RAGGED>
using MaskfilterStemsSamplesArg = std::conditional_t<RAGGED, const MaskfilterUnit* __restrict__, long long>;   // (restrict: the table is read with scalar loads)
template <int LOG2W, bool REST, bool RAGGED>
__global__ __launch_bounds__((MaskfilterCfg<LOG2W, true>::NT)) void k_maskfilter_stems(const float* __restrict__ x, const float* __restrict__ mask,
                                                                                   const float* __restrict__ window, const float2* __restrict__ tw_g,
                                                                                   float* __restrict__ out, MaskfilterStemsSamplesArg<RAGGED> n_samples, long long mask_clip, int n_stems,
                                                                                   int n_blocks, int seg_blocks, int n_segs, long long n_units, float gain) {
    using K = MaskfilterCfg<LOG2W, true>;
    using C = typename K::C;
    constexpr int E = K::E, H = K::H, W = K::W, F = K::F, P = K::P, HE = E / 2;
    extern __shared__ float2 smem[];
    const int tid = threadIdx.x, lane = tid & (P - 1), f = __builtin_amdgcn_readfirstlane(tid / P);
    float2* const buf = smem + f * C::PITCH;
    float* const carry0 = reinterpret_cast<float*>(smem + K::OFF_CARRY);
    float* const carry1 = reinterpret_cast<float*>(smem + K::SLOTS) - H;   // carry s >= 1 at carry1 + s H
    float2* const tw = smem + K::OFF_TW;
    for (int i = tid; i < C::TW; i += K::NT) tw[i] = tw_g[i];
    __syncthreads();
    // samples of the unit's clip: the kernel's argument, or (RAGGED) the field of the unit's record
#define CLIP_N rg_pick<RAGGED>(rc.n_samples, n_samples)
    unsigned clip_bytes = 0, mask_bytes = 0;   // (clips below 2^28 samples: the launcher)
    if constexpr (!RAGGED) {
        clip_bytes = (unsigned)(n_samples * 4);
        mask_bytes = (unsigned)(mask_clip * 4);
    }
    constexpr int st = (H + 1) * 4;   // bytes from frame to frame of a mask
    const int blocks_out = n_stems + (REST ? 1 : 0);

    // The deal (zafx_overlap_walk.hpp); RAGGED counts in 32 bits (the launcher keeps the units below 2^31), as k_maskfilter does and for its reasons
    using Cnt = std::conditional_t<RAGGED, unsigned, long long>;
    const Cnt n_all = (Cnt)n_units, n_deal = deal_rounds<RAGGED>(n_all);
    unsigned round = 0;
    for (Cnt w = blockIdx.x; w < n_deal; w += gridDim.x, ++round) {
        Cnt u;
        if (!deal_unit<RAGGED>(w, round, n_all, u)) continue;
        MaskfilterUnit rc{};   // (RAGGED only) uniform: read with scalar loads
        int b0, b1;
        const float* xc;
        float* oc;
        const float* mc;
        if constexpr (RAGGED) {
            rc = read_unit(n_samples, u);
            if (rc.b1 <= rc.b0) continue;   // a value-initialised record: no blocks (uniform)
            b0 = rc.b0, b1 = rc.b1;
            n_blocks = (int)((rc.n_samples + H - 1) / H);
            mask_clip = (long long)(n_blocks + 1) * (H + 1);   // a stem's mask: frames 0 .. n_blocks, compact
            xc = x + rc.in_off, mc = mask + rc.mask_off, oc = out + rc.out_off;
            clip_bytes = (unsigned)(rc.n_samples * 4);
            mask_bytes = (unsigned)(n_blocks + 1) * (unsigned)((H + 1) * 4);
        } else {
            const EqualUnit eu = equal_unit(u, n_segs, seg_blocks, n_blocks);
            b0 = eu.b0, b1 = eu.b1;
            xc = x + eu.clip * n_samples;
            oc = out + eu.clip * blocks_out * n_samples;
            mc = mask + eu.clip * n_stems * mask_clip;
        }
        const int q0 = b0 >> 1, q1 = b1 >> 1;
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(xc, clip_bytes);
        for (int qt = q0; qt <= q1; qt += F) {
            const int q = qt + f;
            const bool live = q <= q1;   // (wave-uniform)
            float2 v[E], zk[HE], zn[HE], zh = make_float2(0.f, 0.f);
            float raw[E], ma[HE], mb[HE], mah = 0.f, mbh = 0.f;
            // a frame beyond the clip's last (n_blocks) has no mask: the offset -4 reads zero, as does everything outside the stem's mask
            const bool has_a = live && 2 * q <= n_blocks, has_b = live && 2 * q + 1 <= n_blocks;
            const int m0 = lane * 4 + 2 * q * st;
            auto load_mask = [&](int s) {   // stem s < n_stems (uniform)
                const __amdgpu_buffer_rsrc_t rm = make_rsrc(mc + s * mask_clip, mask_bytes);
#pragma unroll
                for (int m = 0; m < HE; ++m) {
                    ma[m] = buf_load_f32(rm, has_a ? m0 + P * m * 4 : -4);
                    mb[m] = buf_load_f32(rm, has_b ? m0 + P * m * 4 + st : -4);
                }
                if (lane == 0) {   // bin H
                    mah = buf_load_f32(rm, has_a ? H * 4 + 2 * q * st : -4);
                    mbh = buf_load_f32(rm, has_b ? H * 4 + 2 * q * st + st : -4);
                }
            };
            {
                const int s0 = (2 * q - 1) * H + lane;
                float xr[E + HE];
#pragma unroll
                for (int i = 0; i < E + HE; ++i) xr[i] = buf_load_f32(rs, live ? (s0 + P * i) * 4 : -4);
                load_mask(0);
#pragma unroll
                for (int i = 0; i < E; ++i) {
                    const float wv = window[lane + P * i];
                    v[i] = make_float2(xr[i] * wv, xr[i + HE] * wv);
                }
                if constexpr (REST) {
#pragma unroll
                    for (int i = 0; i < E; ++i) raw[i] = xr[i];   // the inputs of blocks 2q - 1 (i < HE) and 2q: the rest is subtracted from them in place
                }
                fft_frame<LOG2W, K::LOG2E>(v, buf, lane, tw);
                // the spectrum of this lane's pairs (k, W - k), k = lane + P m < H, and lane 0's bin H: kept through the stems
#pragma unroll
                for (int m = 0; m < HE; ++m) {
                    const int k = lane + P * m, kn = (W - k) & (W - 1);
                    zk[m] = buf[phys_t<C::PS>(k)];
                    zn[m] = buf[phys_t<C::PS>(kn)];
                }
                if (lane == 0) zh = buf[phys_t<C::PS>(H)];
            }
            const bool writes_odd = live && q > q0;          // block 2q - 1
            const bool writes_even = live && 2 * q < b1;     // block 2q
            const bool hands_on = f == F - 1 && live && q < q1;   // the tile's last transform: its imaginary second half is the next tile's carry
            for (int s = 0; s < n_stems; ++s) {
#pragma unroll
                for (int m = 0; m < HE; ++m) {
                    const int k = lane + P * m, kn = (W - k) & (W - 1);
                    float2 ck, cn;
                    maskfilter_pair(zk[m], zn[m], ma[m], mb[m], ck, cn);
                    buf[phys_t<C::PS>(k)] = center_swap(ck);
                    buf[phys_t<C::PS>(kn)] = center_swap(cn);
                }
                if (lane == 0) {
                    float2 ck, cn;
                    maskfilter_pair(zh, zh, mah, mbh, ck, cn);
                    buf[phys_t<C::PS>(H)] = center_swap(ck);
                }
                if (s + 1 < n_stems) load_mask(s + 1);   // (uniform) the next stem's values arrive under this stem's inverse
                frame_sync<P>();
                regs_read<LOG2W, K::LOG2E>(v, buf, lane);
                frame_sync<P>();
                fft_frame<LOG2W, K::LOG2E>(v, buf, lane, tw);
                lds_barrier();   // A: every transform of the tile lies in LDS, swapped: .y = masked frame 2q, .x = masked frame 2q + 1
                float* const carry = s ? carry1 + s * H : carry0;
                float yo[HE], ye[HE], keep[HE];
                if (writes_odd) {
                    const float2* const prev = f > 0 ? buf - C::PITCH : nullptr;
#pragma unroll
                    for (int i = 0; i < HE; ++i) {
                        const int n = lane + P * i;
                        const float a = f > 0 ? prev[phys_t<C::PS>(H + n)].x : carry[n];
                        yo[i] = (a + buf[phys_t<C::PS>(n)].y) * gain;
                    }
                }
                if (writes_even) {
#pragma unroll
                    for (int i = 0; i < HE; ++i) {
                        const int n = lane + P * i;
                        ye[i] = (buf[phys_t<C::PS>(H + n)].y + buf[phys_t<C::PS>(n)].x) * gain;
                    }
                }
                if (hands_on) {
#pragma unroll
                    for (int i = 0; i < HE; ++i) keep[i] = buf[phys_t<C::PS>(H + lane + P * i)].x;
                }
                lds_barrier();   // B: the frames and the stem's carry have been read; the next stem's pairs may overwrite the frames
                if (hands_on) {
#pragma unroll
                    for (int i = 0; i < HE; ++i) carry[lane + P * i] = keep[i];
                }
                float* const os = oc + (long long)s * CLIP_N;
                if (writes_odd) {
                    const long long sm = (long long)(2 * q - 1) * H + lane;
#pragma unroll
                    for (int i = 0; i < HE; ++i) {
                        if (sm + P * i < CLIP_N) {   // nothing is written at or beyond sample N
                            os[sm + P * i] = yo[i];
                            if constexpr (REST) raw[i] = raw[i] - yo[i];
                        }
                    }
                }
                if (writes_even) {
                    const long long sm = (long long)(2 * q) * H + lane;
#pragma unroll
                    for (int i = 0; i < HE; ++i) {
                        if (sm + P * i < CLIP_N) {
                            os[sm + P * i] = ye[i];
                            if constexpr (REST) raw[HE + i] = raw[HE + i] - ye[i];
                        }
                    }
                }
            }
            if constexpr (REST) {   // block S: what the stems left of the samples
                float* const orest = oc + (long long)n_stems * CLIP_N;
                if (writes_odd) {
                    const long long sm = (long long)(2 * q - 1) * H + lane;
#pragma unroll
                    for (int i = 0; i < HE; ++i)
                        if (sm + P * i < CLIP_N) orest[sm + P * i] = raw[i];
                }
                if (writes_even) {
                    const long long sm = (long long)(2 * q) * H + lane;
#pragma unroll
                    for (int i = 0; i < HE; ++i)
                        if (sm + P * i < CLIP_N) orest[sm + P * i] = raw[HE + i];
                }
            }
        }
        lds_barrier();   // the next unit's first tile writes the frames this one's last tile may still be reading
    }
#undef CLIP_N
}

static const char* const kMaskfilterStemsRaggedName = "k_maskfilter_stems_ragged";

// One launch of k_maskfilter_stems<LOG2W, REST, RAGGED>; the slots follow the stems' LDS size.  Equal-length: n clips of n_samples samples each,
// cut by k_maskfilter's rule (maskfilter_equal_segments).  RAGGED (zafx_execute_masked_stems_ragged): the n units of d_units, which come cut and
// ordered from the host (maskfilter_cut_units under the stems' slots).
template <int LOG2W, bool REST, bool RAGGED>
static hipError_t run_maskfilter_stems(const zafx_plan& pl, const float* x, const float* mask, float* out, const MaskfilterUnit* d_units, int64_t n, int64_t n_samples,
                                       int n_stems) {
    using K = MaskfilterCfg<LOG2W, true>;
    static_assert(maskfilter_stems_smem<LOG2W>(kMaskfilterMaxStems) <= (size_t)kMaxLdsBytes, "k_maskfilter_stems: frames + carries + tables exceed LDS");
    auto kern = k_maskfilter_stems<LOG2W, REST, RAGGED>;
    const size_t smem = maskfilter_stems_smem<LOG2W>(n_stems);
    const long long slots = lds_slots(pl.n_cus, smem);
    if constexpr (RAGGED) {
        return launch_walk<LOG2W>(pl, kern, kMaskfilterStemsRaggedName, K::NT, smem, n, slots, x, mask, pl.d_window, pl.d_tw_pass, out, d_units, 0LL, n_stems, 0, 0, 0);
    } else {
        const int64_t n_blocks = n <= 0 ? 0 : (n_samples + K::H - 1) / K::H;
        const int64_t mask_clip = (n_blocks + 1) * (K::H + 1);
        const EqualSegments cut = n_blocks <= 0 ? EqualSegments{0, 0} : maskfilter_equal_segments(n_blocks, n, K::F, slots);
        return launch_walk<LOG2W>(pl, kern, kMaskfilterStemsKernel, K::NT, smem, cut.segs * n, slots, x, mask, pl.d_window, pl.d_tw_pass, out, (long long)n_samples,
                                  (long long)mask_clip, n_stems, (int)n_blocks, (int)cut.seg_blocks, (int)cut.segs);
    }
}

template <bool RAGGED>
static hipError_t dispatch_maskfilter_stems(const zafx_plan& pl, const float* x, const float* mask, float* out, const MaskfilterUnit* d_units, int64_t n,
                                            int64_t n_samples, int n_stems) {
    hipError_t e = hipErrorInvalidValue;
    if (!dispatch_log2w(pl.log2nf, [&](auto lw) {
            constexpr int L = decltype(lw)::value;
            e = pl.kind == ZAFX_MASKFILTER_REST ? run_maskfilter_stems<L, true, RAGGED>(pl, x, mask, out, d_units, n, n_samples, n_stems)
                                                : run_maskfilter_stems<L, false, RAGGED>(pl, x, mask, out, d_units, n, n_samples, n_stems);
        }))
        set_error("mask filter: window_length must be 256, 512, 1024 or 2048");
    return e;
}

hipError_t launch_maskfilter_stems(const zafx_plan& pl, const float* x, const float* mask, float* out, int64_t n_clips, int64_t n_samples, int64_t n_stems) {
    if (const char* why = maskfilter_stems_refusal(route_call(pl, x, out, n_clips, n_samples, 0), n_stems)) {
        set_error(why);
        return hipErrorInvalidValue;
    }
    return dispatch_maskfilter_stems<false>(pl, x, mask, out, nullptr, n_clips, n_samples, (int)n_stems);
}

bool maskfilter_stems_launch_shape(const zafx_plan& pl, int n_stems, int* tile_transforms, long long* slots) {
    if (n_stems < 1 || n_stems > kMaskfilterMaxStems) return false;
    *tile_transforms = maskfilter_tile_transforms(pl.log2nf);
    return dispatch_log2w(pl.log2nf, [&](auto lw) { *slots = lds_slots(pl.n_cus, maskfilter_stems_smem<decltype(lw)::value>(n_stems)); });
}

hipError_t launch_maskfilter_stems_ragged(const zafx_plan& pl, const float* x, const float* mask, float* out, const MaskfilterUnit* d_units, long long n_units,
                                          int64_t n_stems) {
    if (pl.layout != ZAFX_LAYOUT_TF || n_stems < 1 || n_stems > kMaskfilterMaxStems) {   // (the entry point has said why: maskfilter_stems_ragged_refusal)
        set_error("mask filter stems: ZAFX_LAYOUT_TF plans and 1 .. 8 stems only");
        return hipErrorInvalidValue;
    }
    if (n_units >= (1LL << 31)) {
        set_error("mask filter stems: ragged batch too large for one launch (units >= 2^31)");
        return hipErrorInvalidValue;
    }
    return dispatch_maskfilter_stems<true>(pl, x, mask, out, d_units, n_units, 0, (int)n_stems);
}

}  // namespace zafx
