// zafx_maskfilter_pcm.hip -- k_maskfilter_pcm and k_maskfilter_stereo_pcm: the mask filter on 16-bit PCM (zafx_execute_masked_pcm,
// zafx_execute_masked_pcm_ragged; ZAFX_MASKFILTER / ZAFX_MASKFILTER_REST plans of ZAFX_LAYOUT_TF).
//
// The samples are int16 in the kernels' own loads and, with OUT16, in their stores: no float32 staging array on either side.  Sibling kernels
// of k_maskfilter's TF form (zafx_maskfilter.hip) and of k_maskfilter_stereo (zafx_maskfilter_stereo.hip) in a translation unit of their own,
// not a sample-type parameter of those: their instantiations keep their code objects (DESIGN.md 4.12 "PCM").  The walk, the tiles, the carry,
// the barriers, the mask reads, the unit records and the cuts are those kernels'; read their headers for them.  What differs
// (zafx_maskfilter_pcm.hpp has the arithmetic):
//
//   * Loads.  Mono: a 2-byte buffer load per sample behind the clip's descriptor of 2 N bytes; the range check still supplies the zeros in
//     front of sample 0 and from N on, and a dead transform reads offset -2.  Stereo: one dword per sample frame, (L, R) as two int16, behind
//     a descriptor of 4 N bytes; a dead frame reads -4.  A sample s enters as s / 32768, exact in float32: everything between the loads and the
//     stores computes the float kernel's values on the normalised clip, bit for bit.
//   * Stores.  float32 (OUT16 = false): the float kernel's, rest = x / 32768 - y included.  int16 (OUT16): q(y) (pcm_quantise), 2-byte stores
//     mono, one dword per sample frame stereo; the rest comes from the integers, clamp(x - q(y)) (pcm_rest).  Guarded by N as there.
//   * REST keeps the frame's samples as loaded: integers, one register per sample (mono) or per sample frame (stereo).
//   * Arrays: mono on 2 bytes, stereo int16 on 4 (the sample-frame grid), float32 on 4; the entry points refuse anything else.
#include <algorithm>

#include "zafx_maskfilter_cfg.hpp"
#include "zafx_maskfilter_pcm.hpp"
#include "zafx_units.hpp"
#include "zafx_overlap_walk.hpp"

namespace zafx {

__device__ __forceinline__ int buf_load_i16(__amdgpu_buffer_rsrc_t r, int voff) {   // sign-extended
    return (int)(short)__builtin_amdgcn_raw_buffer_load_b16(r, voff, 0, 0);
}

template <bool RAGGED>
using PcmSamplesArg = std::conditional_t<RAGGED, const MaskfilterUnit* __restrict__, long long>;   // (as MaskfilterSamplesArg, zafx_maskfilter.hip)
template <bool OUT16>
using PcmOut = std::conditional_t<OUT16, short, float>;   // a mono output sample
template <bool OUT16>
using PcmOut2 = std::conditional_t<OUT16, int, float2>;   // a stereo output sample frame

// ---- k_maskfilter_pcm: mono clips under one real mask in ZAFX_LAYOUT_TF.  k_maskfilter<LOG2W, REST, true, RAGGED> with int16 samples in and
// int16 (OUT16) or float32 samples out; arguments, units and launch shape are that kernel's (mask_pitch is H + 1 in TF: not passed).
template <int LOG2W, bool REST, bool RAGGED, bool OUT16>
__global__ __launch_bounds__((MaskfilterCfg<LOG2W, true>::NT)) void k_maskfilter_pcm(const short* __restrict__ x, const float* __restrict__ mask,
                                                                                const float* __restrict__ window, const float2* __restrict__ tw_g,
                                                                                PcmOut<OUT16>* __restrict__ out, PcmSamplesArg<RAGGED> n_samples, long long mask_clip,
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
    unsigned clip_bytes = 0, mask_bytes = 0;   // (the launcher keeps every clip below 2^28 samples, which keeps its mask below 2^31 bytes)
    constexpr int sk = 4, st = (H + 1) * 4;    // bytes from bin to bin and from frame to frame
    if constexpr (!RAGGED) {
        clip_bytes = (unsigned)(n_samples * 2);
        mask_bytes = (unsigned)(mask_clip * 4);
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
        const short* xc;
        long long mo;   // the first element of the clip's mask
        PcmOut<OUT16>* oc;
        if constexpr (RAGGED) {
            rc = read_unit(n_samples, u);
            if (rc.b1 <= rc.b0) continue;   // a value-initialised record: no blocks (uniform)
            b0 = rc.b0, b1 = rc.b1;
            n_blocks = (int)((rc.n_samples + H - 1) / H);
            xc = x + rc.in_off, mo = rc.mask_off, oc = out + rc.out_off;
            clip_bytes = (unsigned)(rc.n_samples * 2);
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
            float2 v[E];
            float ma[HE], mb[HE], mah = 0.f, mbh = 0.f;
            int raw[E];
            {
                // samples in front of the clip and at or behind its end read as zero: the descriptor's range check does both, and a
                // transform that is not needed reads nothing but zeros (its threads still meet the others at every frame_sync)
                const int s0 = (2 * q - 1) * H + lane;
                int xi[E + HE];
#pragma unroll
                for (int i = 0; i < E + HE; ++i) xi[i] = buf_load_i16(rs, live ? (s0 + P * i) * 2 : -2);
                // the mask of this lane's pairs, in flight under the forward transform.  Frames beyond the clip's last (n_blocks) have none:
                // the offset -4 reads zero, as does everything outside the clip's mask.
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
                float xr[E + HE];
#pragma unroll
                for (int i = 0; i < E + HE; ++i) xr[i] = pcm_sample(xi[i]);
#pragma unroll
                for (int i = 0; i < E; ++i) {
                    const float wv = window[lane + P * i];
                    v[i] = make_float2(xr[i] * wv, xr[i + HE] * wv);
                }
                if constexpr (REST) {
#pragma unroll
                    for (int i = 0; i < E; ++i) raw[i] = xi[i];   // the inputs of blocks 2q - 1 (i < HE) and 2q, which this wave writes
                }
                fft_frame<LOG2W, K::LOG2E>(v, buf, lane, tw);
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
            // one sample of a block and, REST, of the block N samples behind it: the float kernel's stores, or (OUT16) the quantised ones
            auto put = [&](long long s, float y, int xs) {
                if constexpr (OUT16) {
                    const int qy = pcm_quantise(y);
                    oc[s] = (short)qy;
                    if constexpr (REST) oc[CLIP_N + s] = (short)pcm_rest(xs, qy);
                } else {
                    oc[s] = y;
                    if constexpr (REST) oc[CLIP_N + s] = pcm_sample(xs) - y;
                }
            };
            if (writes_odd) {
                const long long s = (long long)(2 * q - 1) * H + lane;
#pragma unroll
                for (int i = 0; i < HE; ++i)
                    if (s + P * i < CLIP_N) put(s + P * i, yo[i], REST ? raw[i] : 0);   // nothing is written at or beyond sample N
            }
            if (writes_even) {
                const long long s = (long long)(2 * q) * H + lane;
#pragma unroll
                for (int i = 0; i < HE; ++i)
                    if (s + P * i < CLIP_N) put(s + P * i, ye[i], REST ? raw[HE + i] : 0);
            }
        }
        lds_barrier();   // the next unit's first tile writes the frames this one's last tile may still be reading
    }
#undef CLIP_N
}

// ---- k_maskfilter_stereo_pcm: interleaved stereo clips under one mask for both channels or one per channel.
// k_maskfilter_stereo<LOG2W, REST, PER_CHANNEL, RAGGED> with int16 sample frames in and int16 (OUT16) or float32 sample frames out.
template <int LOG2W, bool REST, bool PER_CHANNEL, bool RAGGED, bool OUT16>
__global__ __launch_bounds__(MaskfilterStereoCfg<LOG2W>::NT) void k_maskfilter_stereo_pcm(const int* __restrict__ x, const float* __restrict__ mask,
                                                                                            const float* __restrict__ window, const float2* __restrict__ tw_g,
                                                                                            PcmOut2<OUT16>* __restrict__ out, PcmSamplesArg<RAGGED> n_samples, int n_blocks,
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
#define CLIP_N rg_pick<RAGGED>(rc.n_samples, n_samples)
    // (the launcher keeps every clip below 2^28 sample frames, 2^27 with a mask per channel: the clip and its masks stay below 2^31 bytes)
    unsigned clip_bytes = 0, mask_bytes = 0;
    if constexpr (!RAGGED) {
        clip_bytes = (unsigned)(n_samples * 4);
        mask_bytes = (unsigned)(n_blocks + 1) * (unsigned)st;
    }

    const long long n_deal = deal_rounds<RAGGED>(n_units);   // (zafx_overlap_walk.hpp: the deal)
    int round = 0;
    for (long long w = blockIdx.x; w < n_deal; w += gridDim.x, ++round) {
        long long u;
        if (!deal_unit<RAGGED>(w, round, n_units, u)) continue;   // (the last round may be short; uniform)
        MaskfilterUnit rc{};   // (RAGGED only) uniform: read with scalar loads
        int b0, b1;            // blocks [b0, b1) need frames b0 .. b1
        const int* xc;
        long long mo;          // the first float of the clip's mask(s)
        PcmOut2<OUT16>* oc;
        if constexpr (RAGGED) {
            rc = read_unit(n_samples, u);
            b0 = rc.b0, b1 = rc.b1;
            xc = x + rc.in_off, mo = rc.mask_off, oc = out + rc.out_off;
            clip_bytes = (unsigned)(rc.n_samples * 4);
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
            float2 v[E];
            int raw[HE];
            float m0[HE], m1[HE], m0h = 0.f, m1h = 0.f;
            {
                // samples in front of the clip and at or behind its end read as zero: the descriptor's range check does both, and a
                // frame that is not needed reads nothing but zeros (its threads still meet the others at every frame_sync)
                const int s0 = (j - 1) * H + lane;
                int xi[E];
#pragma unroll
                for (int i = 0; i < E; ++i) xi[i] = buf_load_i32(rs, live ? (s0 + P * i) * 4 : -4);
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
                    for (int i = 0; i < HE; ++i) raw[i] = xi[i];   // the frame's first half is the input of block j - 1, which this wave writes
                }
#pragma unroll
                for (int i = 0; i < E; ++i) v[i] = make_float2(pcm_sample(pcm_left(xi[i])), pcm_sample(pcm_right(xi[i])));
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
                        if constexpr (OUT16) {
                            const int ql = pcm_quantise(y[i].x), qr = pcm_quantise(y[i].y);
                            oc[s + P * i] = pcm_pack(ql, qr);
                            if constexpr (REST) oc[CLIP_N + s + P * i] = pcm_pack(pcm_rest(pcm_left(raw[i]), ql), pcm_rest(pcm_right(raw[i]), qr));
                        } else {
                            oc[s + P * i] = y[i];
                            if constexpr (REST)
                                oc[CLIP_N + s + P * i] = csub(make_float2(pcm_sample(pcm_left(raw[i])), pcm_sample(pcm_right(raw[i]))), y[i]);
                        }
                    }
                }
            }
        }
        lds_barrier();   // the next unit's first tile writes the frames this one's last tile may still be reading
    }
#undef CLIP_N
}

// ---- the launchers.  `out16`: the output holds int16 samples (out_sample_bytes 2) instead of float32 ones (4).

// One launch of k_maskfilter_pcm<LOG2W, REST, RAGGED, OUT16>: equal-length clips cut here as run_maskfilter cuts them (zafx_maskfilter.hip), or
// (RAGGED) the n units of d_units.
template <int LOG2W, bool REST, bool RAGGED, bool OUT16>
static hipError_t run_pcm(const zafx_plan& pl, const void* x, const float* mask, void* out, const MaskfilterUnit* d_units, int64_t n, int64_t n_samples) {
    using K = MaskfilterCfg<LOG2W, true>;
    auto kern = k_maskfilter_pcm<LOG2W, REST, RAGGED, OUT16>;
    const short* xi = static_cast<const short*>(x);
    PcmOut<OUT16>* o = static_cast<PcmOut<OUT16>*>(out);
    const long long slots = lds_slots(pl.n_cus, K::SMEM);
    if constexpr (RAGGED) {
        return launch_walk<LOG2W>(pl, kern, kMaskfilterPcmRaggedKernel, K::NT, K::SMEM, n, slots, xi, mask, pl.d_window, pl.d_tw_pass, o, d_units, 0LL, 0, 0, 0);
    } else {
        const int64_t n_blocks = n <= 0 ? 0 : (n_samples + K::H - 1) / K::H;
        const int64_t mask_clip = (n_blocks + 1) * (K::H + 1);
        const EqualSegments cut = n_blocks <= 0 ? EqualSegments{0, 0} : maskfilter_equal_segments(n_blocks, n, K::F, slots);
        return launch_walk<LOG2W>(pl, kern, kMaskfilterPcmKernel, K::NT, K::SMEM, cut.segs * n, slots, xi, mask, pl.d_window, pl.d_tw_pass, o, (long long)n_samples,
                                  (long long)mask_clip, (int)n_blocks, (int)cut.seg_blocks, (int)cut.segs);
    }
}

// One launch of k_maskfilter_stereo_pcm<LOG2W, REST, PER_CHANNEL, RAGGED, OUT16>, cut as run_stereo cuts (zafx_maskfilter_stereo.hip).
template <int LOG2W, bool REST, bool PER_CHANNEL, bool RAGGED, bool OUT16>
static hipError_t run_stereo_pcm(const zafx_plan& pl, const void* x, const float* mask, void* out, const MaskfilterUnit* d_units, int64_t n, int64_t n_samples) {
    using K = MaskfilterStereoCfg<LOG2W>;
    auto kern = k_maskfilter_stereo_pcm<LOG2W, REST, PER_CHANNEL, RAGGED, OUT16>;
    const int* xi = static_cast<const int*>(x);
    PcmOut2<OUT16>* o = static_cast<PcmOut2<OUT16>*>(out);
    const long long slots = lds_slots(pl.n_cus, K::SMEM);
    if constexpr (RAGGED) {
        return launch_walk<LOG2W>(pl, kern, kMaskfilterStereoPcmRaggedKernel, K::NT, K::SMEM, n, slots, xi, mask, pl.d_window, pl.d_tw_pass, o, d_units, 0, 0, 0);
    } else {
        const int64_t n_blocks = n <= 0 ? 0 : (n_samples + K::H - 1) / K::H;
        const EqualSegments cut = n_blocks <= 0 ? EqualSegments{0, 0} : center_equal_segments(n_blocks, n, K::F, slots);
        return launch_walk<LOG2W>(pl, kern, kMaskfilterStereoPcmKernel, K::NT, K::SMEM, cut.segs * n, slots, xi, mask, pl.d_window, pl.d_tw_pass, o, (long long)n_samples,
                                  (int)n_blocks, (int)cut.seg_blocks, (int)cut.segs);
    }
}

// channels 1: k_maskfilter_pcm; 2: k_maskfilter_stereo_pcm under mask_channels masks
template <bool RAGGED>
static hipError_t dispatch_pcm(const zafx_plan& pl, const void* x, const float* mask, void* out, const MaskfilterUnit* d_units, int64_t n, int64_t n_samples,
                               int channels, int mask_channels, bool out16) {
    const bool rest = pl.kind == ZAFX_MASKFILTER_REST, pc = mask_channels == 2;
    hipError_t e = hipErrorInvalidValue;
    if (!dispatch_log2w(pl.log2nf, [&](auto lw) {
            constexpr int L = decltype(lw)::value;
            auto with = [&](auto r, auto o16) {
                constexpr bool R = decltype(r)::value, O = decltype(o16)::value;
                if (channels == 1) e = run_pcm<L, R, RAGGED, O>(pl, x, mask, out, d_units, n, n_samples);
                else if (pc) e = run_stereo_pcm<L, R, true, RAGGED, O>(pl, x, mask, out, d_units, n, n_samples);
                else e = run_stereo_pcm<L, R, false, RAGGED, O>(pl, x, mask, out, d_units, n, n_samples);
            };
            if (rest) out16 ? with(std::true_type{}, std::true_type{}) : with(std::true_type{}, std::false_type{});
            else out16 ? with(std::false_type{}, std::true_type{}) : with(std::false_type{}, std::false_type{});
        }))
        set_error("mask filter: window_length must be 256, 512, 1024 or 2048");
    return e;
}

// The launchers ask the refusal themselves as well as the entry points: no caller reaches a kernel with an FT plan, another channel count or
// a clip at the bound.
hipError_t launch_maskfilter_pcm(const zafx_plan& pl, const void* x, const float* mask, void* out, int64_t n_clips, int64_t n_samples, int channels,
                                 int mask_channels, bool out16) {
    const char* why = maskfilter_pcm_channels_refusal(channels, mask_channels);
    if (!why) why = maskfilter_form_refusal(maskfilter_pcm_form(channels), route_call(pl, x, out, n_clips, n_samples, 0), channels == 2 ? mask_channels : 0, true);
    if (why) {
        set_error(why);
        return hipErrorInvalidValue;
    }
    return dispatch_pcm<false>(pl, x, mask, out, nullptr, n_clips, n_samples, channels, mask_channels, out16);
}

hipError_t launch_maskfilter_pcm_ragged(const zafx_plan& pl, const void* x, const float* mask, void* out, const MaskfilterUnit* d_units, long long n_units,
                                        int channels, int mask_channels, bool out16) {
    const char* why = maskfilter_pcm_channels_refusal(channels, mask_channels);
    if (!why && pl.layout != ZAFX_LAYOUT_TF) why = maskfilter_pcm_form(channels).wrong_layout;
    if (!why && n_units >= (1LL << 31)) why = "mask filter: ragged batch too large for one launch (units >= 2^31)";
    if (why) {
        set_error(why);
        return hipErrorInvalidValue;
    }
    return dispatch_pcm<true>(pl, x, mask, out, d_units, n_units, 0, channels, mask_channels, out16);
}

}  // namespace zafx
