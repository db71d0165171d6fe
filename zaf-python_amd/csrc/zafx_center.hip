// zafx_center.hip -- k_center: the center / sides extraction of zaf.istft's example (zaf.py:155-198) in one kernel.
//
// Stereo STFT, the two time-frequency masks, both ISTFTs and sides = input - center without a spectrum ever leaving the CU
// (zafx_center.hpp has the arithmetic and the mask's one departure from the reference).  Structure (what it shares with
// k_maskfilter and k_maskfilter_stems: zafx_overlap_walk.hpp):
//
//   * An interleaved stereo sample frame (L, R) IS one complex point of z = L + i R: a frame of W sample frames is loaded as W
//     float2, multiplied by the window and transformed as ONE W-point complex FFT.  Up to W = 1024 64 lanes own a frame (W / 64
//     points per lane) and every exchange of the transform is wave-local (frame_sync<64>: no workgroup barrier inside a transform);
//     at W = 2048 two wavefronts share a frame (16 points per lane: with 32 the transform does not fit 256 registers) and
//     frame_sync is the workgroup's barrier, so every wave runs every tile's transforms, on zeros where its frame is not needed.
//   * Split, mask and re-pack run in place on the pairs (k, W-k) of the LDS frame; the inverse transform is the forward core on
//     the swapped parts.  Its real part is the center's left channel, its imaginary part the right one.
//   * A workgroup of center_tile_frames(log2 W) frames' threads walks the frames of one segment of a clip in order, a tile of that many frames at
//     a time.  Only step_length = W/2 exists (zaf.stft pads W/2 in front, zaf.istft trims W - H: the two agree at no other hop), so an
//     output block b (sample frames b H .. b H + H - 1) is the second half of frame b plus the first half of frame b + 1: the wave
//     of frame b + 1 writes it, taking the other half from its neighbour's LDS frame or, for the first frame of a tile, from the
//     carry the previous tile left in LDS.  A segment starts by transforming the frame in front of its first block (one halo frame
//     per segment), so it produces the same bits wherever it starts; every sample is the sum of exactly two terms.
//   * SIDES: the lanes that write block b hold its input samples already (the first half of frame b + 1, before the window).
//   * RAGGED (zafx_execute_center_ragged): clips of different lengths.  The walk is the same; a unit's clip -- the base and the length
//     its descriptor is built from, the base of its output -- and its blocks come from the unit's record of a device table
//     (CenterUnit, zafx_units.hpp: the host cuts the batch) instead of from clip * n_samples and seg * seg_blocks.  A descriptor
//     per clip pads every clip with zeros even where the next clip's samples lie right behind it.
#include <algorithm>

#include "zafx_center.hpp"
#include "zafx_units.hpp"
#include "zafx_overlap_walk.hpp"

namespace zafx {

template <int LOG2W>
struct CenterCfg {
    static constexpr int LOG2E = center_log2e(LOG2W);
    using C = FftCfg<LOG2W, LOG2E>;
    static constexpr int W = 1 << LOG2W, H = W / 2, E = C::E, P = C::P, F = center_tile_frames(LOG2W), NT = P * F;
    static_assert(P == 64 || P == 128, "k_center: one or two wavefronts per frame");
    // LDS (float2 slots): F padded frames | the carry (second half of the tile's last frame, H points) | the pass tables
    static constexpr int OFF_CARRY = F * C::PITCH, OFF_TW = OFF_CARRY + H, SLOTS = OFF_TW + C::TW;
    static constexpr size_t SMEM = (size_t)SLOTS * 8;
    static_assert(SMEM <= (size_t)kMaxLdsBytes, "k_center: frames + carry + tables exceed LDS");
};

// One segment = blocks [seg * seg_blocks, min(n_blocks, (seg + 1) * seg_blocks)) of one clip; unit u = clip * n_segs + seg.
// RAGGED: `n_samples` carries the table of unit records (SamplesArg, zafx_internal.hpp: the equal-length instantiations keep their kernel
// arguments byte for byte), unit u is record u, and n_blocks / seg_blocks / n_segs are not used.
template <bool RAGGED>
using CenterSamplesArg = std::conditional_t<RAGGED, const CenterUnit* __restrict__, long long>;   // (restrict: the table is read with scalar loads)
template <int LOG2W, bool SIDES, bool RAGGED>
__global__ __launch_bounds__(CenterCfg<LOG2W>::NT) void k_center(const float2* __restrict__ x, const float* __restrict__ window, const float2* __restrict__ tw_g,
                                                                   float2* __restrict__ out, CenterSamplesArg<RAGGED> n_samples, int n_blocks,
                                                                   int seg_blocks, int n_segs, long long n_units, float gain) {
    using K = CenterCfg<LOG2W>;
    using C = typename K::C;
    constexpr int E = K::E, H = K::H, W = K::W, F = K::F, P = K::P, HE = E / 2;
    extern __shared__ float2 smem[];
    const int tid = threadIdx.x, lane = tid & (P - 1), f = __builtin_amdgcn_readfirstlane(tid / P);   // lane: the thread's place among its frame's P
    float2* const buf = smem + f * C::PITCH;
    float2* const carry = smem + K::OFF_CARRY;
    float2* const tw = smem + K::OFF_TW;
    for (int i = tid; i < C::TW; i += K::NT) tw[i] = tw_g[i];
    __syncthreads();
    // sample frames of the unit's clip: the kernel's argument, or (RAGGED) the field of the unit's record
#define CLIP_N rg_pick<RAGGED>(rc.n_samples, n_samples)
    unsigned clip_bytes = 0;   // (the launcher keeps every clip below 2^28 sample frames)
    if constexpr (!RAGGED) clip_bytes = (unsigned)(n_samples * 8);

    const long long n_deal = deal_rounds<RAGGED>(n_units);   // (zafx_overlap_walk.hpp: the deal)
    int round = 0;
    for (long long w = blockIdx.x; w < n_deal; w += gridDim.x, ++round) {
        long long u;
        if (!deal_unit<RAGGED>(w, round, n_units, u)) continue;   // (the last round may be short; uniform)
        CenterUnit rc{};   // (RAGGED only) uniform: read with scalar loads
        int b0, b1;        // blocks [b0, b1) need frames b0 .. b1
        const float2* xc;
        float2* oc;
        if constexpr (RAGGED) {
            rc = read_unit(n_samples, u);
            b0 = rc.b0, b1 = rc.b1;
            xc = x + rc.in_off;
            oc = out + rc.out_off;
            clip_bytes = (unsigned)(rc.n_samples * 8);
        } else {
            const EqualUnit eu = equal_unit(u, n_segs, seg_blocks, n_blocks);
            b0 = eu.b0, b1 = eu.b1;
            xc = x + eu.clip * n_samples;
            oc = out + eu.clip * n_samples * (SIDES ? 2 : 1);
        }
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(xc, clip_bytes);
        for (int j0 = b0; j0 <= b1; j0 += F) {
            const int j = j0 + f;              // this wave's frame: sample frames (j - 1) H .. (j + 1) H - 1
            const bool live = j <= b1;         // (wave-uniform)
            float2 v[E], raw[HE];
            {
                // samples in front of the clip and at or behind its end read as zero: the descriptor's range check does both, and a
                // frame that is not needed reads nothing but zeros (its threads still meet the others at every frame_sync)
                // (8-byte loads here and 8-byte stores below at the clip's base plus a multiple of 8 bytes: a base at 4 mod 8 -- include/zafx.h
                // allows any 4-byte boundary -- makes them misaligned for float2, which global and buffer accesses take on this hardware in its
                // unaligned access mode; tests/test_gpu_arena.py runs such bases.  Not something to "fix" by rounding the base.)
                const int s0 = (j - 1) * H + lane;
#pragma unroll
                for (int i = 0; i < E; ++i) v[i] = buf_load_f32x2(rs, live ? (s0 + P * i) * 8 : -8);
                if constexpr (SIDES) {
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
                    center_pair(buf[pk], buf[pn], ck, cn);
                    buf[pk] = center_swap(ck);
                    buf[pn] = center_swap(cn);
                }
                if (lane == 0) {
                    const int ph = phys_t<C::PS>(H);
                    float2 ck, cn;
                    center_pair(buf[ph], buf[ph], ck, cn);
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
                        if constexpr (SIDES) oc[CLIP_N + s + P * i] = csub(raw[i], y[i]);
                    }
                }
            }
        }
        lds_barrier();   // the next unit's first tile writes the frames this one's last tile may still be reading
    }
#undef CLIP_N
}

static const char* const kCenterName = kCenterKernel;   // (zafx_routes.hpp)
static const char* const kCenterRaggedName = "k_center_ragged";
const char* center_kernel_name() { return kCenterName; }

// One launch of k_center<LOG2W, SIDES, RAGGED>.  Equal-length: n clips of n_samples sample frames each, cut here (center_equal_segments).
// RAGGED (zafx_execute_center_ragged): the n units of d_units, which come cut and ordered from the host (center_cut_units).
template <int LOG2W, bool SIDES, bool RAGGED>
static hipError_t run_center(const zafx_plan& pl, const float2* x, float2* out, const CenterUnit* d_units, int64_t n, int64_t n_samples) {
    using K = CenterCfg<LOG2W>;
    auto kern = k_center<LOG2W, SIDES, RAGGED>;
    const long long slots = lds_slots(pl.n_cus, K::SMEM);
    if constexpr (RAGGED) {
        return launch_walk<LOG2W>(pl, kern, kCenterRaggedName, K::NT, K::SMEM, n, slots, x, pl.d_window, pl.d_tw_pass, out, d_units, 0, 0, 0);
    } else {
        const int64_t n_blocks = (n_samples + K::H - 1) / K::H;
        if (n_blocks <= 0 || n <= 0) return hipSuccess;
        const EqualSegments cut = center_equal_segments(n_blocks, n, K::F, slots);
        return launch_walk<LOG2W>(pl, kern, kCenterName, K::NT, K::SMEM, cut.segs * n, slots, x, pl.d_window, pl.d_tw_pass, out, (long long)n_samples,
                                  (int)n_blocks, (int)cut.seg_blocks, (int)cut.segs);
    }
}

// log2 of the complex FFT length = log2(W): a sample frame is one complex point
template <bool RAGGED>
static hipError_t dispatch_center(const zafx_plan& pl, const float* x, float* out, const CenterUnit* d_units, int64_t n, int64_t n_samples) {
    const float2* xi = reinterpret_cast<const float2*>(x);
    float2* o = reinterpret_cast<float2*>(out);
    hipError_t e = hipErrorInvalidValue;
    if (!dispatch_log2w(pl.log2nf, [&](auto lw) {
            constexpr int L = decltype(lw)::value;
            e = pl.kind == ZAFX_CENTER_SIDES ? run_center<L, true, RAGGED>(pl, xi, o, d_units, n, n_samples) : run_center<L, false, RAGGED>(pl, xi, o, d_units, n, n_samples);
        }))
        set_error("center / sides: window_length must be 256, 512, 1024 or 2048");
    return e;
}

hipError_t launch_center(const zafx_plan& pl, const float* x, float* out, int64_t n_clips, int64_t n_samples) {
    if (center_clip_refused(route_call(pl, x, out, n_clips, n_samples, 0))) {
        set_error("center / sides: clips of 2^28 sample frames and more are not supported");
        return hipErrorInvalidValue;
    }
    return dispatch_center<false>(pl, x, out, nullptr, n_clips, n_samples);
}

bool center_launch_shape(const zafx_plan& pl, int* tile_frames, long long* slots) {
    *tile_frames = center_tile_frames(pl.log2nf);
    return dispatch_log2w(pl.log2nf, [&](auto lw) { *slots = lds_slots(pl.n_cus, CenterCfg<decltype(lw)::value>::SMEM); });
}

hipError_t launch_center_ragged(const zafx_plan& pl, const float* x, float* out, const CenterUnit* d_units, long long n_units) {
    if (n_units >= (1LL << 31)) {
        set_error("center / sides: ragged batch too large for one launch (units >= 2^31)");
        return hipErrorInvalidValue;
    }
    return dispatch_center<true>(pl, x, out, d_units, n_units, 0);
}

}  // namespace zafx
