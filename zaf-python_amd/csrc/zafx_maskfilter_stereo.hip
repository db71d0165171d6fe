// zafx_maskfilter_stereo.hip -- k_maskfilter_stereo: STFT, the caller's real time-frequency mask(s) and ISTFT of interleaved stereo clips in
// one kernel (zafx_execute_masked_stereo, zafx_execute_masked_stereo_ragged; ZAFX_MASKFILTER / ZAFX_MASKFILTER_REST plans of ZAFX_LAYOUT_TF).
//
// y[:, c] = istft(concat(m_c, m_c[-2:0:-1]) * stft(x[:, c], w, W/2), w, W/2)[0:N] for both channels without a spectrum ever leaving the CU;
// REST: rest = x - y behind it.  zafx_maskfilter_stereo.hpp has the arithmetic and what the packing means for the two channels.  A kernel of
// its own beside k_center, not a parameter of it: that one's instantiations keep their code objects (DESIGN.md 4.12 "Stereo").
//
// The walk is k_center's (zafx_center.hip): a sample frame (L, R) is one complex point of z = L + i R, a frame of W sample
// frames one W-point complex transform; units of (clip, blocks [b0, b1)) need frames b0 .. b1, the first one the halo; tiles of
// center_tile_frames frames; k_center's LDS (frames, carry, pass tables -- nothing more); barriers A / B, the carry handed on, stores
// guarded by N.  What differs:
//
//   * The mask.  Element (frame t, bin k) of a clip's shared mask lies at t (H + 1) + k; with a mask per channel the frame's L row lies
//     directly in front of its R row: (t, c, k) at (2 t + c)(H + 1) + k.  One descriptor per clip's mask.  A lane's bins k = lane + P m,
//     m < E / 2, are 64 consecutive floats of the frame's row per load instruction, lane 0 takes bin H as well; the loads are issued behind
//     the sample loads and in front of the forward transform and arrive under it.  A frame that is not live reads offset -4: zero.
//     Every live frame j <= b1 <= n_blocks has a mask: T = n_blocks + 1.
//   * Between the transforms: maskfilter_stereo_pair (a mask per channel: split, scale, re-pack) or maskfilter_stereo_pair_shared (one mask:
//     Z[k] and Z[W-k] scaled, no split) on the pairs (k, W-k) of the LDS frame.
//   * RAGGED: the unit's record is a MaskfilterUnit (zafx_units.hpp; cut by maskfilter_stereo_cut_units with k_center's rule), which carries
//     mask_off, the first float32 element of the clip's mask(s).  Offsets and lengths of samples count sample frames.
#include <algorithm>

#include "zafx_maskfilter_cfg.hpp"
#include "zafx_units.hpp"
#include "zafx_overlap_walk.hpp"

namespace zafx {

// One segment = blocks [seg * seg_blocks, min(n_blocks, (seg + 1) * seg_blocks)) of one clip; unit u = clip * n_segs + seg; the masks of a clip
// are (n_blocks + 1) x (PER_CHANNEL ? 2 : 1) rows of H + 1 floats, clips back to back.
// RAGGED: `n_samples` carries the table of unit records (as k_center's CenterSamplesArg), unit u is record u, and n_blocks / seg_blocks /
// n_segs are not used.
template <bool RAGGED>
using StereoSamplesArg = std::conditional_t<RAGGED, const MaskfilterUnit* __restrict__, long long>;   // (restrict: the table is read with scalar loads)
template <int LOG2W, bool REST, bool PER_CHANNEL, bool RAGGED>
__global__ __launch_bounds__(MaskfilterStereoCfg<LOG2W>::NT) void k_maskfilter_stereo(const float2* __restrict__ x, const float* __restrict__ mask,
                                                                                        const float* __restrict__ window, const float2* __restrict__ tw_g,
                                                                                        float2* __restrict__ out, StereoSamplesArg<RAGGED> n_samples, int n_blocks,
                                                                                        int seg_blocks, int n_segs, long long n_units, float gain) {
    using K = MaskfilterStereoCfg<LOG2W>;
    using C = typename K::C;
    constexpr int E = K::E, H = K::H, W = K::W, F = K::F, P = K::P, HE = E / 2;
    constexpr int ROW = (H + 1) * 4, st = PER_CHANNEL ? 2 * ROW : ROW;   // bytes of a mask row, and from frame to frame
    extern __shared__ float2 smem[];
    const int tid = threadIdx.x, lane = tid & (P - 1), f = __builtin_amdgcn_readfirstlane(tid / P);   // lane: the thread's place among its frame's P
    float2* const buf = smem + f * C::PITCH;
    float2* const carry = smem + K::OFF_CARRY;
    float2* const tw = smem + K::OFF_TW;
    for (int i = tid; i < C::TW; i += K::NT) tw[i] = tw_g[i];
    __syncthreads();
    // sample frames of the unit's clip: the kernel's argument, or (RAGGED) the field of the unit's record
#define CLIP_N rg_pick<RAGGED>(rc.n_samples, n_samples)
    // (the launcher keeps every clip below 2^28 sample frames, 2^27 with a mask per channel: the clip and its masks stay below 2^31 bytes)
    unsigned clip_bytes = 0, mask_bytes = 0;
    if constexpr (!RAGGED) {
        clip_bytes = (unsigned)(n_samples * 8);
        mask_bytes = (unsigned)(n_blocks + 1) * (unsigned)st;
    }

    const long long n_deal = deal_rounds<RAGGED>(n_units);   // (zafx_overlap_walk.hpp: the deal)
    int round = 0;
    for (long long w = blockIdx.x; w < n_deal; w += gridDim.x, ++round) {
        long long u;
        if (!deal_unit<RAGGED>(w, round, n_units, u)) continue;   // (the last round may be short; uniform)
        MaskfilterUnit rc{};   // (RAGGED only) uniform: read with scalar loads
        int b0, b1;            // blocks [b0, b1) need frames b0 .. b1
        const float2* xc;
        long long mo;          // the first float of the clip's mask(s)
        float2* oc;
        if constexpr (RAGGED) {
            rc = read_unit(n_samples, u);
            b0 = rc.b0, b1 = rc.b1;
            xc = x + rc.in_off, mo = rc.mask_off, oc = out + rc.out_off;
            clip_bytes = (unsigned)(rc.n_samples * 8);
            mask_bytes = (unsigned)((rc.n_samples + H - 1) / H + 1) * (unsigned)st;   // the masks end with the last row of frame n_blocks
        } else {
            const EqualUnit eu = equal_unit(u, n_segs, seg_blocks, n_blocks);
            b0 = eu.b0, b1 = eu.b1;
            xc = x + eu.clip * n_samples;
            oc = out + eu.clip * n_samples * (REST ? 2 : 1);
            mo = eu.clip * ((long long)(n_blocks + 1) * (st / 4));
        }
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(xc, clip_bytes);
        const __amdgpu_buffer_rsrc_t rm = make_rsrc(mask + mo, mask_bytes);
        for (int j0 = b0; j0 <= b1; j0 += F) {
            const int j = j0 + f;              // this wave's frame: sample frames (j - 1) H .. (j + 1) H - 1
            const bool live = j <= b1;         // (wave-uniform)
            float2 v[E], raw[HE];
            float m0[HE], m1[HE], m0h = 0.f, m1h = 0.f;
            {
                // samples in front of the clip and at or behind its end read as zero: the descriptor's range check does both, and a
                // frame that is not needed reads nothing but zeros (its threads still meet the others at every frame_sync)
                // (8-byte loads here and 8-byte stores below at the clip's base plus a multiple of 8 bytes, as in k_center: a base at 4 mod 8
                // makes them misaligned for float2, which this hardware takes in its unaligned access mode.  Not something to "fix" by
                // rounding the base.)
                const int s0 = (j - 1) * H + lane;
#pragma unroll
                for (int i = 0; i < E; ++i) v[i] = buf_load_f32x2(rs, live ? (s0 + P * i) * 8 : -8);
                // the mask values of this lane's pairs, in flight under the forward transform; a frame that is not live reads zero
                const int mj = j * st + lane * 4;
#pragma unroll
                for (int m = 0; m < HE; ++m) {
                    m0[m] = buf_load_f32(rm, live ? mj + P * m * 4 : -4);
                    if constexpr (PER_CHANNEL) m1[m] = buf_load_f32(rm, live ? mj + ROW + P * m * 4 : -4);
                }
                if (lane == 0) {   // bin H
                    m0h = buf_load_f32(rm, live ? j * st + H * 4 : -4);
                    if constexpr (PER_CHANNEL) m1h = buf_load_f32(rm, live ? j * st + ROW + H * 4 : -4);
                }
                if constexpr (REST) {
#pragma unroll
                    for (int i = 0; i < HE; ++i) raw[i] = v[i];   // the frame's first half is the input of block j - 1, which this wave writes
                }
#pragma unroll
                for (int i = 0; i < E; ++i) v[i] = cscale(v[i], window[lane + P * i]);
                fft_frame<LOG2W, K::LOG2E>(v, buf, lane, tw);
                // pairs (k, W - k), k = lane + P m < H; k = 0 pairs with itself, and lane 0 takes k = H as well
#pragma unroll
                for (int m = 0; m < HE; ++m) {
                    const int k = lane + P * m, kn = (W - k) & (W - 1);
                    const int pk = phys_t<C::PS>(k), pn = phys_t<C::PS>(kn);
                    float2 ck, cn;
                    if constexpr (PER_CHANNEL) maskfilter_stereo_pair(buf[pk], buf[pn], m0[m], m1[m], ck, cn);
                    else maskfilter_stereo_pair_shared(buf[pk], buf[pn], m0[m], ck, cn);
                    buf[pk] = center_swap(ck);
                    buf[pn] = center_swap(cn);
                }
                if (lane == 0) {
                    const int ph = phys_t<C::PS>(H);
                    float2 ck, cn;
                    if constexpr (PER_CHANNEL) maskfilter_stereo_pair(buf[ph], buf[ph], m0h, m1h, ck, cn);
                    else maskfilter_stereo_pair_shared(buf[ph], buf[ph], m0h, ck, cn);
                    buf[ph] = center_swap(ck);
                }
                frame_sync<P>();
                regs_read<LOG2W, K::LOG2E>(v, buf, lane);
                frame_sync<P>();
                fft_frame<LOG2W, K::LOG2E>(v, buf, lane, tw);
            }
            lds_barrier();   // A: every frame of the tile lies in LDS
            // block j - 1 = second half of frame j - 1 + first half of frame j
            const int b = j - 1;
            const bool writes = live && b >= b0 && (f > 0 || j0 > b0);
            const bool hands_on = f == F - 1 && live && j < b1;   // the tile's last frame: its second half is the next tile's carry
            float2 y[HE], keep[HE];
            if (writes) {
                const float2* const prev = f > 0 ? buf - C::PITCH : nullptr;
#pragma unroll
                for (int i = 0; i < HE; ++i) {
                    const int n = lane + P * i;
                    const float2 a = f > 0 ? prev[phys_t<C::PS>(H + n)] : carry[n];
                    y[i] = center_swap(cscale(cadd(a, buf[phys_t<C::PS>(n)]), gain));
                }
            }
            if (hands_on) {
#pragma unroll
                for (int i = 0; i < HE; ++i) keep[i] = buf[phys_t<C::PS>(H + lane + P * i)];
            }
            lds_barrier();   // B: the frames and the carry have been read
            if (hands_on) {
#pragma unroll
                for (int i = 0; i < HE; ++i) carry[lane + P * i] = keep[i];
            }
            if (writes) {
                const long long s = (long long)b * H + lane;
#pragma unroll
                for (int i = 0; i < HE; ++i) {
                    if (s + P * i < CLIP_N) {   // nothing is written at or beyond sample frame N
                        oc[s + P * i] = y[i];
                        if constexpr (REST) oc[CLIP_N + s + P * i] = csub(raw[i], y[i]);
                    }
                }
            }
        }
        lds_barrier();   // the next unit's first tile writes the frames this one's last tile may still be reading
    }
#undef CLIP_N
}

// One launch of k_maskfilter_stereo<LOG2W, REST, PER_CHANNEL, RAGGED>.  Equal-length: n clips of n_samples sample frames each, cut here as
// k_center's are (center_equal_segments).  RAGGED: the n units of d_units, which come cut and ordered from the host (maskfilter_stereo_cut_units).
template <int LOG2W, bool REST, bool PER_CHANNEL, bool RAGGED>
static hipError_t run_stereo(const zafx_plan& pl, const float2* x, const float* mask, float2* out, const MaskfilterUnit* d_units, int64_t n, int64_t n_samples) {
    using K = MaskfilterStereoCfg<LOG2W>;
    auto kern = k_maskfilter_stereo<LOG2W, REST, PER_CHANNEL, RAGGED>;
    const long long slots = lds_slots(pl.n_cus, K::SMEM);
    if constexpr (RAGGED) {
        return launch_walk<LOG2W>(pl, kern, kMaskfilterStereoRaggedKernel, K::NT, K::SMEM, n, slots, x, mask, pl.d_window, pl.d_tw_pass, out, d_units, 0, 0, 0);
    } else {
        const int64_t n_blocks = n <= 0 ? 0 : (n_samples + K::H - 1) / K::H;
        const EqualSegments cut = n_blocks <= 0 ? EqualSegments{0, 0} : center_equal_segments(n_blocks, n, K::F, slots);
        return launch_walk<LOG2W>(pl, kern, kMaskfilterStereoKernel, K::NT, K::SMEM, cut.segs * n, slots, x, mask, pl.d_window, pl.d_tw_pass, out, (long long)n_samples,
                                  (int)n_blocks, (int)cut.seg_blocks, (int)cut.segs);
    }
}

// log2 of the complex FFT length = log2(W): a sample frame is one complex point
template <bool RAGGED>
static hipError_t dispatch_stereo(const zafx_plan& pl, const float* x, const float* mask, float* out, const MaskfilterUnit* d_units, int64_t n, int64_t n_samples,
                                  int mask_channels) {
    const float2* xi = reinterpret_cast<const float2*>(x);
    float2* o = reinterpret_cast<float2*>(out);
    const bool rest = pl.kind == ZAFX_MASKFILTER_REST, pc = mask_channels == 2;
    hipError_t e = hipErrorInvalidValue;
    if (!dispatch_log2w(pl.log2nf, [&](auto lw) {
            constexpr int L = decltype(lw)::value;
            if (rest) e = pc ? run_stereo<L, true, true, RAGGED>(pl, xi, mask, o, d_units, n, n_samples) : run_stereo<L, true, false, RAGGED>(pl, xi, mask, o, d_units, n, n_samples);
            else e = pc ? run_stereo<L, false, true, RAGGED>(pl, xi, mask, o, d_units, n, n_samples) : run_stereo<L, false, false, RAGGED>(pl, xi, mask, o, d_units, n, n_samples);
        }))
        set_error("mask filter: window_length must be 256, 512, 1024 or 2048");
    return e;
}

// The launchers ask the refusal themselves as well as the entry points: no caller reaches the kernel with an FT plan, another mask_channels or
// a clip at the bound.
hipError_t launch_maskfilter_stereo(const zafx_plan& pl, const float* x, const float* mask, float* out, int64_t n_clips, int64_t n_samples, int mask_channels) {
    if (const char* why = maskfilter_stereo_refusal(route_call(pl, x, out, n_clips, n_samples, 0), mask_channels)) {
        set_error(why);
        return hipErrorInvalidValue;
    }
    return dispatch_stereo<false>(pl, x, mask, out, nullptr, n_clips, n_samples, mask_channels);
}

bool maskfilter_stereo_launch_shape(const zafx_plan& pl, int* tile_frames, long long* slots) {
    *tile_frames = maskfilter_stereo_tile_frames(pl.log2nf);
    return dispatch_log2w(pl.log2nf, [&](auto lw) { *slots = lds_slots(pl.n_cus, MaskfilterStereoCfg<decltype(lw)::value>::SMEM); });
}

hipError_t launch_maskfilter_stereo_ragged(const zafx_plan& pl, const float* x, const float* mask, float* out, const MaskfilterUnit* d_units, long long n_units,
                                           int mask_channels) {
    const bool bad_call = pl.layout != ZAFX_LAYOUT_TF || (mask_channels != 1 && mask_channels != 2);
    if (bad_call || n_units >= (1LL << 31)) {
        set_error(bad_call ? "stereo mask filter: masks in ZAFX_LAYOUT_TF only, mask_channels 1 or 2" : "mask filter: ragged batch too large for one launch (units >= 2^31)");
        return hipErrorInvalidValue;
    }
    return dispatch_stereo<true>(pl, x, mask, out, d_units, n_units, 0, mask_channels);
}

}  // namespace zafx
