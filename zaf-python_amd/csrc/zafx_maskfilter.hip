// zafx_maskfilter.hip -- k_maskfilter: STFT, the caller's real time-frequency mask and ISTFT of mono clips in one kernel.
//
// y = istft(concat(m, m[-2:0:-1]) * stft(x, w, W/2), w, W/2)[0:N] (zaf.py:185-195 with a mask of the caller's) without a spectrum ever
// leaving the CU; REST: rest = x - y behind it.  zafx_maskfilter.hpp has the arithmetic.  Structure, on k_center's plan
// (zafx_center.hip) of segments, tiles and a carry in LDS:
//
//   * Two neighbouring frames of one clip are ONE W-point complex transform: transform q holds frame 2q (sample frames (2q - 1) H ..) in
//     its real part and frame 2q + 1 (2q H ..) in its imaginary part.  The second half of frame 2q IS the first half of frame 2q + 1, so
//     a lane loads 3 E / 2 samples for its E complex points.  No two clips ever share a transform.
//   * Split, mask and re-pack run in place on the pairs (k, W-k) of the LDS frame (maskfilter_pair) with the mask values of a lane's
//     pairs, m[k, 2q] and m[k, 2q + 1].  ZAFX_LAYOUT_TF: 64 lanes read 64 consecutive floats of a frame's row, behind the samples and in
//     front of the forward transform, so the values arrive under it.  ZAFX_LAYOUT_FT: a lane's two values are 8 bytes of ITS row -- read that
//     way a load instruction touches 64 lines and every line comes from HBM about five times --, so every second tile the
//     whole workgroup fetches the next FS frames of every row, FS lanes to a row (64 or 128 contiguous bytes), into a stage in LDS, and
//     the lanes take their pairs' values from there.  These loads are waited for where they are issued, not under the transform.
//     A frame beyond the clip's last (an odd frame count pairs the last frame with zeros) reads no mask: its mask is 0.
//   * The inverse is the forward core on the swapped parts.  Output block b (samples b H .. b H + H - 1) is the second half of frame b plus
//     the first half of frame b + 1: block 2q comes from transform q alone, block 2q - 1 from the imaginary part of transform q - 1 -- the
//     neighbour's LDS frame, or the carry the previous tile left -- and the real part of transform q.  The lanes of transform q write both.
//   * A segment is an even number of blocks, so it starts on a transform of its own and needs nothing in front; one that ends on an even
//     block runs one transform more for that block's second term (the halo).  Every transform's inputs are the clip's own samples and mask
//     columns whatever the segment, so a clip has the same bits however it is cut.
//   * RAGGED (zafx_execute_masked_ragged): clips of different lengths.  The walk is the same; a unit's clip -- the base and the length of its
//     samples, the base, pitch and extent of its mask, the base of its output -- and its blocks come from the unit's record of a device
//     table (MaskfilterUnit, zafx_units.hpp: the host cuts the batch into even-sized segments) instead of from clip * n_samples,
//     clip * mask_clip and seg * seg_blocks.  A descriptor per clip and per mask pads every clip with zeros and ends every mask at its own
//     last column, even where the next clip's samples or mask lie right behind.
#include <algorithm>

#include "zafx_maskfilter_cfg.hpp"
#include "zafx_units.hpp"
#include "zafx_overlap_walk.hpp"

namespace zafx {

// One segment = blocks [seg * seg_blocks, min(n_blocks, (seg + 1) * seg_blocks)) of one clip, seg_blocks even; unit u = clip * n_segs + seg.
// mask: element (bin k, frame t) of a clip at k * mask_pitch + t (FT) or t * (H + 1) + k (TF); clips mask_clip elements apart.
// RAGGED: `n_samples` carries the table of unit records (the equal-length instantiations keep their kernel arguments byte for byte, as
// k_center's do: CenterSamplesArg), unit u is record u, and mask_clip / mask_pitch / n_blocks / seg_blocks / n_segs are not used.
template <bool RAGGED>
using MaskfilterSamplesArg = std::conditional_t<RAGGED, const MaskfilterUnit* __restrict__, long long>;   // (restrict: the table is read with scalar loads)
template <int LOG2W, bool REST, bool TF, bool RAGGED>
__global__ __launch_bounds__((MaskfilterCfg<LOG2W, TF>::NT)) void k_maskfilter(const float* __restrict__ x, const float* __restrict__ mask,
                                                                           const float* __restrict__ window, const float2* __restrict__ tw_g,
                                                                           float* __restrict__ out, MaskfilterSamplesArg<RAGGED> n_samples, long long mask_clip, int mask_pitch,
                                                                           int n_blocks, int seg_blocks, int n_segs, long long n_units, float gain) {
    using K = MaskfilterCfg<LOG2W, TF>;
    using C = typename K::C;
    constexpr int E = K::E, H = K::H, W = K::W, F = K::F, P = K::P, HE = E / 2, FS = K::FS, SP = K::SP;
    extern __shared__ float2 smem[];
    const int tid = threadIdx.x, lane = tid & (P - 1), f = __builtin_amdgcn_readfirstlane(tid / P);   // lane: the thread's place among its transform's P
    float2* const buf = smem + f * C::PITCH;
    float* const carry = reinterpret_cast<float*>(smem + K::OFF_CARRY);
    float2* const tw = smem + K::OFF_TW;
    float* const stage = reinterpret_cast<float*>(smem + K::OFF_STAGE);   // (ZAFX_LAYOUT_FT only)
    for (int i = tid; i < C::TW; i += K::NT) tw[i] = tw_g[i];
    __syncthreads();
    // samples of the unit's clip: the kernel's argument, or (RAGGED) the field of the unit's record
#define CLIP_N rg_pick<RAGGED>(rc.n_samples, n_samples)
    unsigned clip_bytes = 0, mask_bytes = 0;   // (the launcher keeps every clip below 2^28 samples, which keeps its mask below 2^31 bytes)
    int sk = TF ? 4 : 0;                       // bytes from bin to bin ...
    constexpr int st = TF ? (H + 1) * 4 : 4;   // ... and from frame to frame
    if constexpr (!RAGGED) {
        clip_bytes = (unsigned)(n_samples * 4);
        mask_bytes = (unsigned)(mask_clip * 4);
        sk = TF ? 4 : mask_pitch * 4;
    }

    // The deal (zafx_overlap_walk.hpp), as k_center's.
    // (RAGGED counts its units in 32 bits -- the launcher keeps them below 2^31 --: the loop's tests are then scalar compares; 64-bit ones are
    // vector compares that hold n_deal in a VGPR pair through the kernel, and W = 256 / TF has none to spare beside its twin's 64)
    using Cnt = std::conditional_t<RAGGED, unsigned, long long>;
    const Cnt n_all = (Cnt)n_units, n_deal = deal_rounds<RAGGED>(n_all);
    unsigned round = 0;
    for (Cnt w = blockIdx.x; w < n_deal; w += gridDim.x, ++round) {
        Cnt u;
        if (!deal_unit<RAGGED>(w, round, n_all, u)) continue;
        MaskfilterUnit rc{};   // (RAGGED only) uniform: read with scalar loads
        int b0, b1;
        const float* xc;
        long long mo;   // the first element of the clip's mask
        float* oc;
        if constexpr (RAGGED) {
            rc = read_unit(n_samples, u);
            if (rc.b1 <= rc.b0) continue;   // a value-initialised record: no blocks (uniform)
            b0 = rc.b0, b1 = rc.b1;
            n_blocks = (int)((rc.n_samples + H - 1) / H);
            xc = x + rc.in_off, mo = rc.mask_off, oc = out + rc.out_off;
            clip_bytes = (unsigned)(rc.n_samples * 4);
            // the mask ends with its last frame's last bin: FT row H, column n_blocks; TF frame n_blocks, bin H
            mask_bytes = TF ? (unsigned)(n_blocks + 1) * (unsigned)((H + 1) * 4) : ((unsigned)H * (unsigned)rc.mask_pitch + (unsigned)(n_blocks + 1)) * 4u;
            if constexpr (!TF) sk = rc.mask_pitch * 4;
        } else {
            const EqualUnit eu = equal_unit(u, n_segs, seg_blocks, n_blocks);
            b0 = eu.b0, b1 = eu.b1;
            xc = x + eu.clip * n_samples;
            oc = out + eu.clip * n_samples * (REST ? 2 : 1);
            mo = eu.clip * mask_clip;
        }
        const int q0 = b0 >> 1, q1 = b1 >> 1;   // transforms q0 .. q1 hold the frames b0 .. b1 that blocks [b0, b1) need
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(xc, clip_bytes);
        const __amdgpu_buffer_rsrc_t rm = make_rsrc(mask + mo, mask_bytes);
        for (int qt = q0; qt <= q1; qt += F) {
            const int q = qt + f;            // this wave's transform: frames 2q and 2q + 1
            const bool live = q <= q1;       // (wave-uniform)
            float2 v[E];
            float raw[E], ma[HE], mb[HE], mah = 0.f, mbh = 0.f;
            const int qs = q0 + (qt - q0) / (2 * F) * (2 * F);   // first transform of the tile's mask stage (FT)
            {
                // samples in front of the clip and at or behind its end read as zero: the descriptor's range check does both, and a
                // transform that is not needed reads nothing but zeros (its threads still meet the others at every frame_sync)
                const int s0 = (2 * q - 1) * H + lane;
                float xr[E + HE];
#pragma unroll
                for (int i = 0; i < E + HE; ++i) xr[i] = buf_load_f32(rs, live ? (s0 + P * i) * 4 : -4);
                // the mask: TF this lane's pairs, in flight under the forward transform; FT the stage of this tile and the next.  Frames beyond
                // the clip's last (n_blocks) have none: the offset -4 reads zero, as does everything outside the clip's mask.
                if constexpr (TF) {
                    const bool has_a = live && 2 * q <= n_blocks, has_b = live && 2 * q + 1 <= n_blocks;
                    const int m0 = lane * sk + 2 * q * st;
#pragma unroll
                    for (int m = 0; m < HE; ++m) {
                        ma[m] = buf_load_f32(rm, has_a ? m0 + P * m * sk : -4);
                        mb[m] = buf_load_f32(rm, has_b ? m0 + P * m * sk + st : -4);
                    }
                    if (lane == 0) {   // bin H
                        mah = buf_load_f32(rm, has_a ? H * sk + 2 * q * st : -4);
                        mbh = buf_load_f32(rm, has_b ? H * sk + 2 * q * st + st : -4);
                    }
                } else if (qt == qs) {   // (uniform) FT: the whole workgroup fetches frames 2 qs .. 2 qs + FS - 1 of every row, FS lanes to a row
                    constexpr int NL = ((H + 1) * FS + K::NT - 1) / K::NT;
                    float sr[NL];
                    // RAGGED: the row pitch is the unit's, and the NL products r * sk, computed once per unit, would stay in registers through
                    // all of its tiles (30 VGPRs at W = 2048: spills).  The empty statement has them computed here, per stage.
                    int sks = sk;
                    if constexpr (RAGGED) asm volatile("" : "+s"(sks));
#pragma unroll
                    for (int i = 0; i < NL; ++i) {
                        const int e = tid + K::NT * i, r = e / FS, c = e % FS;
                        sr[i] = buf_load_f32(rm, r <= H && 2 * qs + c <= n_blocks ? r * sks + (2 * qs + c) * 4 : -4);
                    }
#pragma unroll
                    for (int i = 0; i < NL; ++i) {
                        const int e = tid + K::NT * i, r = e / FS, c = e % FS;
                        if (r <= H) stage[r * SP + c] = sr[i];
                    }
                    lds_barrier();   // the stage lies in LDS (its last readers met at barrier A of the tile before)
                }
#pragma unroll
                for (int i = 0; i < E; ++i) {
                    const float wv = window[lane + P * i];
                    v[i] = make_float2(xr[i] * wv, xr[i + HE] * wv);
                }
                if constexpr (REST) {
#pragma unroll
                    for (int i = 0; i < E; ++i) raw[i] = xr[i];   // the inputs of blocks 2q - 1 (i < HE) and 2q, which this wave writes
                }
                fft_frame<LOG2W, K::LOG2E>(v, buf, lane, tw);
                if constexpr (!TF) {   // this transform's two columns of the stage (a frame beyond the clip's last was staged as 0)
                    const float* const col = stage + 2 * (q - qs);
#pragma unroll
                    for (int m = 0; m < HE; ++m) {
                        const float2 mm = *reinterpret_cast<const float2*>(col + (lane + P * m) * SP);
                        ma[m] = mm.x, mb[m] = mm.y;
                    }
                    if (lane == 0) mah = col[H * SP], mbh = col[H * SP + 1];
                }
                // pairs (k, W - k), k = lane + P m < H; k = 0 pairs with itself, and lane 0 takes k = H as well
#pragma unroll
                for (int m = 0; m < HE; ++m) {
                    const int k = lane + P * m, kn = (W - k) & (W - 1);
                    const int pk = phys_t<C::PS>(k), pn = phys_t<C::PS>(kn);
                    float2 ck, cn;
                    maskfilter_pair(buf[pk], buf[pn], ma[m], mb[m], ck, cn);
                    buf[pk] = center_swap(ck);
                    buf[pn] = center_swap(cn);
                }
                if (lane == 0) {
                    const int ph = phys_t<C::PS>(H);
                    float2 ck, cn;
                    maskfilter_pair(buf[ph], buf[ph], mah, mbh, ck, cn);
                    buf[ph] = center_swap(ck);
                }
                frame_sync<P>();
                regs_read<LOG2W, K::LOG2E>(v, buf, lane);
                frame_sync<P>();
                fft_frame<LOG2W, K::LOG2E>(v, buf, lane, tw);
            }
            lds_barrier();   // A: every transform of the tile lies in LDS, swapped: .y = masked frame 2q, .x = masked frame 2q + 1
            const bool writes_odd = live && q > q0;          // block 2q - 1 = second half of frame 2q - 1 + first half of frame 2q
            const bool writes_even = live && 2 * q < b1;     // block 2q     = second half of frame 2q + first half of frame 2q + 1
            const bool hands_on = f == F - 1 && live && q < q1;   // the tile's last transform: its imaginary second half is the next tile's carry
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
            lds_barrier();   // B: the frames and the carry have been read
            if (hands_on) {
#pragma unroll
                for (int i = 0; i < HE; ++i) carry[lane + P * i] = keep[i];
            }
            if (writes_odd) {
                const long long s = (long long)(2 * q - 1) * H + lane;
#pragma unroll
                for (int i = 0; i < HE; ++i) {
                    if (s + P * i < CLIP_N) {   // nothing is written at or beyond sample N
                        oc[s + P * i] = yo[i];
                        if constexpr (REST) oc[CLIP_N + s + P * i] = raw[i] - yo[i];
                    }
                }
            }
            if (writes_even) {
                const long long s = (long long)(2 * q) * H + lane;
#pragma unroll
                for (int i = 0; i < HE; ++i) {
                    if (s + P * i < CLIP_N) {
                        oc[s + P * i] = ye[i];
                        if constexpr (REST) oc[CLIP_N + s + P * i] = raw[HE + i] - ye[i];
                    }
                }
            }
        }
        lds_barrier();   // the next unit's first tile writes the frames this one's last tile may still be reading
    }
#undef CLIP_N
}

const char* maskfilter_kernel_name() { return kMaskfilterKernel; }   // (zafx_routes.hpp)

static const char* const kMaskfilterRaggedName = "k_maskfilter_ragged";

// One launch of k_maskfilter<LOG2W, REST, TF, RAGGED>.  Equal-length: n clips of n_samples samples each, cut here (maskfilter_equal_segments).
// RAGGED (zafx_execute_masked_ragged): the n units of d_units, which come cut and ordered from the host (maskfilter_cut_units).
template <int LOG2W, bool REST, bool TF, bool RAGGED>
static hipError_t run_maskfilter(const zafx_plan& pl, const float* x, const float* mask, float* out, const MaskfilterUnit* d_units, int64_t n, int64_t n_samples) {
    using K = MaskfilterCfg<LOG2W, TF>;
    auto kern = k_maskfilter<LOG2W, REST, TF, RAGGED>;
    const long long slots = lds_slots(pl.n_cus, K::SMEM);
    if constexpr (RAGGED) {
        return launch_walk<LOG2W>(pl, kern, kMaskfilterRaggedName, K::NT, K::SMEM, n, slots, x, mask, pl.d_window, pl.d_tw_pass, out, d_units, 0LL, 0, 0, 0, 0);
    } else {
        const int64_t n_blocks = n <= 0 ? 0 : (n_samples + K::H - 1) / K::H;
        const int64_t T = n_blocks + 1, pitch = TF ? K::H + 1 : row_pitch(pl, T);
        const int64_t mask_clip = TF ? T * (K::H + 1) : (int64_t)(K::H + 1) * pitch;
        const EqualSegments cut = n_blocks <= 0 ? EqualSegments{0, 0} : maskfilter_equal_segments(n_blocks, n, K::F, slots);
        return launch_walk<LOG2W>(pl, kern, kMaskfilterKernel, K::NT, K::SMEM, cut.segs * n, slots, x, mask, pl.d_window, pl.d_tw_pass, out, (long long)n_samples,
                                  (long long)mask_clip, (int)pitch, (int)n_blocks, (int)cut.seg_blocks, (int)cut.segs);
    }
}

// log2 of the complex FFT length = log2(W): two frames are one W-point transform
template <bool RAGGED>
static hipError_t dispatch_maskfilter(const zafx_plan& pl, const float* x, const float* mask, float* out, const MaskfilterUnit* d_units, int64_t n, int64_t n_samples) {
    const bool rest = pl.kind == ZAFX_MASKFILTER_REST, tf = pl.layout == ZAFX_LAYOUT_TF;
    hipError_t e = hipErrorInvalidValue;
    if (!dispatch_log2w(pl.log2nf, [&](auto lw) {
            constexpr int L = decltype(lw)::value;
            if (rest) e = tf ? run_maskfilter<L, true, true, RAGGED>(pl, x, mask, out, d_units, n, n_samples) : run_maskfilter<L, true, false, RAGGED>(pl, x, mask, out, d_units, n, n_samples);
            else e = tf ? run_maskfilter<L, false, true, RAGGED>(pl, x, mask, out, d_units, n, n_samples) : run_maskfilter<L, false, false, RAGGED>(pl, x, mask, out, d_units, n, n_samples);
        }))
        set_error("mask filter: window_length must be 256, 512, 1024 or 2048");
    return e;
}

hipError_t launch_maskfilter(const zafx_plan& pl, const float* x, const float* mask, float* out, int64_t n_clips, int64_t n_samples) {
    if (maskfilter_clip_refused(route_call(pl, x, out, n_clips, n_samples, 0))) {
        set_error("mask filter: clips of 2^28 samples and more are not supported");
        return hipErrorInvalidValue;
    }
    return dispatch_maskfilter<false>(pl, x, mask, out, nullptr, n_clips, n_samples);
}

bool maskfilter_launch_shape(const zafx_plan& pl, int* tile_transforms, long long* slots) {
    *tile_transforms = maskfilter_tile_transforms(pl.log2nf);
    return dispatch_log2w(pl.log2nf, [&](auto lw) {
        constexpr int L = decltype(lw)::value;
        *slots = lds_slots(pl.n_cus, pl.layout == ZAFX_LAYOUT_TF ? MaskfilterCfg<L, true>::SMEM : MaskfilterCfg<L, false>::SMEM);
    });
}

hipError_t launch_maskfilter_ragged(const zafx_plan& pl, const float* x, const float* mask, float* out, const MaskfilterUnit* d_units, long long n_units) {
    if (n_units >= (1LL << 31)) {
        set_error("mask filter: ragged batch too large for one launch (units >= 2^31)");
        return hipErrorInvalidValue;
    }
    return dispatch_maskfilter<true>(pl, x, mask, out, d_units, n_units, 0);
}

// ---- k_maskfilter_c: the same walk under a COMPLEX mask (zafx_execute_masked_complex, zafx_execute_masked_complex_ragged), ZAFX_LAYOUT_TF only.
//
// A kernel of its own, not a fifth template parameter of k_maskfilter: that one's 32 instantiations keep their code objects (DESIGN.md 4.12
// "Complex masks").  What differs from k_maskfilter's TF form: the mask is complex64, element (bin k, frame t) of a clip at t (H + 1) + k, so a
// lane's pair k = lane + P m of a frame is ONE 8-byte buffer load (64 lanes: 512 consecutive bytes of the frame's row; the array itself needs
// 4-byte alignment only), issued behind the samples and in front of the forward transform; the pair function is maskfilter_pair_c; and the
// imaginary parts of bins 0 and H -- they pair with themselves -- are dropped from the registers before it, whatever they hold.
// RAGGED: MaskfilterUnit::mask_off counts complex64 elements and mask_pitch is not read.  The launcher keeps every clip below 2^27 samples:
// its mask then lies behind signed 32-bit byte offsets (maskfilter_complex_refusal, zafx_routes.hpp).
template <int LOG2W, bool REST, bool RAGGED>
__global__ __launch_bounds__((MaskfilterCfg<LOG2W, true>::NT)) void k_maskfilter_c(const float* __restrict__ x, const float2* __restrict__ mask,
                                                                              const float* __restrict__ window, const float2* __restrict__ tw_g,
                                                                              float* __restrict__ out, MaskfilterSamplesArg<RAGGED> n_samples, long long mask_clip,
                                                                              int n_blocks, int seg_blocks, int n_segs, long long n_units, float gain) {
    using K = MaskfilterCfg<LOG2W, true>;
    using C = typename K::C;
    constexpr int E = K::E, H = K::H, W = K::W, F = K::F, P = K::P, HE = E / 2;
    extern __shared__ float2 smem[];
    const int tid = threadIdx.x, lane = tid & (P - 1), f = __builtin_amdgcn_readfirstlane(tid / P);   // lane: the thread's place among its transform's P
    float2* const buf = smem + f * C::PITCH;
    float* const carry = reinterpret_cast<float*>(smem + K::OFF_CARRY);
    float2* const tw = smem + K::OFF_TW;
    for (int i = tid; i < C::TW; i += K::NT) tw[i] = tw_g[i];
    __syncthreads();
#define CLIP_N rg_pick<RAGGED>(rc.n_samples, n_samples)
    unsigned clip_bytes = 0, mask_bytes = 0;
    constexpr int sk = 8, st = (H + 1) * 8;   // bytes from bin to bin and from frame to frame
    if constexpr (!RAGGED) {
        clip_bytes = (unsigned)(n_samples * 4);
        mask_bytes = (unsigned)(mask_clip * 8);
    }

    // The deal (zafx_overlap_walk.hpp), counted as k_maskfilter counts it.
    using Cnt = std::conditional_t<RAGGED, unsigned, long long>;
    const Cnt n_all = (Cnt)n_units, n_deal = deal_rounds<RAGGED>(n_all);
    unsigned round = 0;
    for (Cnt w = blockIdx.x; w < n_deal; w += gridDim.x, ++round) {
        Cnt u;
        if (!deal_unit<RAGGED>(w, round, n_all, u)) continue;
        MaskfilterUnit rc{};   // (RAGGED only) uniform: read with scalar loads
        int b0, b1;
        const float* xc;
        long long mo;   // the first complex element of the clip's mask
        float* oc;
        if constexpr (RAGGED) {
            rc = read_unit(n_samples, u);
            if (rc.b1 <= rc.b0) continue;   // a value-initialised record: no blocks (uniform)
            b0 = rc.b0, b1 = rc.b1;
            n_blocks = (int)((rc.n_samples + H - 1) / H);
            xc = x + rc.in_off, mo = rc.mask_off, oc = out + rc.out_off;
            clip_bytes = (unsigned)(rc.n_samples * 4);
            mask_bytes = (unsigned)(n_blocks + 1) * (unsigned)st;   // the mask ends with bin H of frame n_blocks
        } else {
            const EqualUnit eu = equal_unit(u, n_segs, seg_blocks, n_blocks);
            b0 = eu.b0, b1 = eu.b1;
            xc = x + eu.clip * n_samples;
            oc = out + eu.clip * n_samples * (REST ? 2 : 1);
            mo = eu.clip * mask_clip;
        }
        const int q0 = b0 >> 1, q1 = b1 >> 1;   // transforms q0 .. q1 hold the frames b0 .. b1 that blocks [b0, b1) need
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(xc, clip_bytes);
        const __amdgpu_buffer_rsrc_t rm = make_rsrc(mask + mo, mask_bytes);
        for (int qt = q0; qt <= q1; qt += F) {
            const int q = qt + f;            // this wave's transform: frames 2q and 2q + 1
            const bool live = q <= q1;       // (wave-uniform)
            float2 v[E], ma[HE], mb[HE], mah = make_float2(0.f, 0.f), mbh = make_float2(0.f, 0.f);
            float raw[E];
            {
                // samples in front of the clip and at or behind its end read as zero, and a transform that is not needed reads nothing but
                // zeros: the descriptor's range check, as in k_maskfilter
                const int s0 = (2 * q - 1) * H + lane;
                float xr[E + HE];
#pragma unroll
                for (int i = 0; i < E + HE; ++i) xr[i] = buf_load_f32(rs, live ? (s0 + P * i) * 4 : -4);
                // the mask of this lane's pairs, in flight under the forward transform.  Frames beyond the clip's last (n_blocks) have none:
                // the offset -8 reads zero, as does everything outside the clip's mask.
                const bool has_a = live && 2 * q <= n_blocks, has_b = live && 2 * q + 1 <= n_blocks;
                const int m0 = lane * sk + 2 * q * st;
#pragma unroll
                for (int m = 0; m < HE; ++m) {
                    ma[m] = buf_load_f32x2(rm, has_a ? m0 + P * m * sk : -8);
                    mb[m] = buf_load_f32x2(rm, has_b ? m0 + P * m * sk + st : -8);
                }
                if (lane == 0) {   // bin H
                    mah = buf_load_f32x2(rm, has_a ? H * sk + 2 * q * st : -8);
                    mbh = buf_load_f32x2(rm, has_b ? H * sk + 2 * q * st + st : -8);
                }
#pragma unroll
                for (int i = 0; i < E; ++i) {
                    const float wv = window[lane + P * i];
                    v[i] = make_float2(xr[i] * wv, xr[i + HE] * wv);
                }
                if constexpr (REST) {
#pragma unroll
                    for (int i = 0; i < E; ++i) raw[i] = xr[i];   // the inputs of blocks 2q - 1 (i < HE) and 2q, which this wave writes
                }
                fft_frame<LOG2W, K::LOG2E>(v, buf, lane, tw);
                // bins 0 and H pair with themselves: their imaginary parts are discarded (a select, not a product: NaN there does nothing)
                if (lane == 0) ma[0].y = 0.f, mb[0].y = 0.f;
                mah.y = 0.f, mbh.y = 0.f;
                // pairs (k, W - k), k = lane + P m < H; lane 0 takes k = H as well
#pragma unroll
                for (int m = 0; m < HE; ++m) {
                    const int k = lane + P * m, kn = (W - k) & (W - 1);
                    const int pk = phys_t<C::PS>(k), pn = phys_t<C::PS>(kn);
                    float2 ck, cn;
                    maskfilter_pair_c(buf[pk], buf[pn], ma[m], mb[m], ck, cn);
                    buf[pk] = center_swap(ck);
                    buf[pn] = center_swap(cn);
                }
                if (lane == 0) {
                    const int ph = phys_t<C::PS>(H);
                    float2 ck, cn;
                    maskfilter_pair_c(buf[ph], buf[ph], mah, mbh, ck, cn);
                    buf[ph] = center_swap(ck);
                }
                frame_sync<P>();
                regs_read<LOG2W, K::LOG2E>(v, buf, lane);
                frame_sync<P>();
                fft_frame<LOG2W, K::LOG2E>(v, buf, lane, tw);
            }
            lds_barrier();   // A: every transform of the tile lies in LDS, swapped: .y = masked frame 2q, .x = masked frame 2q + 1
            const bool writes_odd = live && q > q0;          // block 2q - 1 = second half of frame 2q - 1 + first half of frame 2q
            const bool writes_even = live && 2 * q < b1;     // block 2q     = second half of frame 2q + first half of frame 2q + 1
            const bool hands_on = f == F - 1 && live && q < q1;   // the tile's last transform: its imaginary second half is the next tile's carry
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
            lds_barrier();   // B: the frames and the carry have been read
            if (hands_on) {
#pragma unroll
                for (int i = 0; i < HE; ++i) carry[lane + P * i] = keep[i];
            }
            if (writes_odd) {
                const long long s = (long long)(2 * q - 1) * H + lane;
#pragma unroll
                for (int i = 0; i < HE; ++i) {
                    if (s + P * i < CLIP_N) {   // nothing is written at or beyond sample N
                        oc[s + P * i] = yo[i];
                        if constexpr (REST) oc[CLIP_N + s + P * i] = raw[i] - yo[i];
                    }
                }
            }
            if (writes_even) {
                const long long s = (long long)(2 * q) * H + lane;
#pragma unroll
                for (int i = 0; i < HE; ++i) {
                    if (s + P * i < CLIP_N) {
                        oc[s + P * i] = ye[i];
                        if constexpr (REST) oc[CLIP_N + s + P * i] = raw[HE + i] - ye[i];
                    }
                }
            }
        }
        lds_barrier();   // the next unit's first tile writes the frames this one's last tile may still be reading
    }
#undef CLIP_N
}

// One launch of k_maskfilter_c<LOG2W, REST, RAGGED>: equal-length clips cut here as run_maskfilter cuts them, or (RAGGED) the n units of d_units.
template <int LOG2W, bool REST, bool RAGGED>
static hipError_t run_maskfilter_c(const zafx_plan& pl, const float* x, const float2* mask, float* out, const MaskfilterUnit* d_units, int64_t n, int64_t n_samples) {
    using K = MaskfilterCfg<LOG2W, true>;
    auto kern = k_maskfilter_c<LOG2W, REST, RAGGED>;
    const long long slots = lds_slots(pl.n_cus, K::SMEM);
    if constexpr (RAGGED) {
        return launch_walk<LOG2W>(pl, kern, kMaskfilterComplexRaggedKernel, K::NT, K::SMEM, n, slots, x, mask, pl.d_window, pl.d_tw_pass, out, d_units, 0LL, 0, 0, 0);
    } else {
        const int64_t n_blocks = n <= 0 ? 0 : (n_samples + K::H - 1) / K::H;
        const int64_t mask_clip = (n_blocks + 1) * (K::H + 1);
        const EqualSegments cut = n_blocks <= 0 ? EqualSegments{0, 0} : maskfilter_equal_segments(n_blocks, n, K::F, slots);
        return launch_walk<LOG2W>(pl, kern, kMaskfilterComplexKernel, K::NT, K::SMEM, cut.segs * n, slots, x, mask, pl.d_window, pl.d_tw_pass, out, (long long)n_samples,
                                  (long long)mask_clip, (int)n_blocks, (int)cut.seg_blocks, (int)cut.segs);
    }
}

template <bool RAGGED>
static hipError_t dispatch_maskfilter_c(const zafx_plan& pl, const float* x, const float2* mask, float* out, const MaskfilterUnit* d_units, int64_t n, int64_t n_samples) {
    const bool rest = pl.kind == ZAFX_MASKFILTER_REST;
    hipError_t e = hipErrorInvalidValue;
    if (!dispatch_log2w(pl.log2nf, [&](auto lw) {
            constexpr int L = decltype(lw)::value;
            e = rest ? run_maskfilter_c<L, true, RAGGED>(pl, x, mask, out, d_units, n, n_samples) : run_maskfilter_c<L, false, RAGGED>(pl, x, mask, out, d_units, n, n_samples);
        }))
        set_error("mask filter: window_length must be 256, 512, 1024 or 2048");
    return e;
}

// The launchers ask the refusal themselves as well as the entry points: no caller reaches the kernel with an FT plan or a clip of 2^27 samples.
hipError_t launch_maskfilter_complex(const zafx_plan& pl, const float* x, const float2* mask, float* out, int64_t n_clips, int64_t n_samples) {
    if (const char* why = maskfilter_complex_refusal(route_call(pl, x, out, n_clips, n_samples, 0))) {
        set_error(why);
        return hipErrorInvalidValue;
    }
    return dispatch_maskfilter_c<false>(pl, x, mask, out, nullptr, n_clips, n_samples);
}

hipError_t launch_maskfilter_complex_ragged(const zafx_plan& pl, const float* x, const float2* mask, float* out, const MaskfilterUnit* d_units, long long n_units) {
    if (pl.layout != ZAFX_LAYOUT_TF || n_units >= (1LL << 31)) {
        set_error(pl.layout != ZAFX_LAYOUT_TF ? "complex mask filter: masks in ZAFX_LAYOUT_TF only" : "mask filter: ragged batch too large for one launch (units >= 2^31)");
        return hipErrorInvalidValue;
    }
    return dispatch_maskfilter_c<true>(pl, x, mask, out, d_units, n_units, 0);
}

}  // namespace zafx
