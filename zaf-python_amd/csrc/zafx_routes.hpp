// zafx_routes.hpp -- which kernel an equal-length float32 call runs, and which launch a ragged batch takes: the one place that decides it.
//
// Plain C++17, no HIP, no getenv: hipcc compiles it into the library (the launchers of zafx_stft.hip, zafx_mdct.hip, zafx_mel.hip, zafx_cqt.hip
// and zafx_center.hip fill a RouteCall -- route_call, zafx_internal.hpp -- ask the family's function once and switch on the answer; the ragged
// entry points of zafx_capi.cpp add a RaggedBatch, filled in the pass that builds the clips' records), g++ compiles it into
// tests/host_emu/routes_emu.cpp, and tests/test_routes_host.py holds that program to the conditions restated in Python (tests/long_clips.py
// BOUNDS) and to the kernels recorded on the GPU (tests/golden/call_routes.json, tests/golden/ragged_routes.json).
//
// Every condition stands here once, under a name; a condition two routes share is one function both call.  The inequalities, constants
// and the order of the tests are those the launchers had inline (profiles/routes_notes.md lists the ones that look inconsistent).
// Out of scope: the equal-length float64 and Bluestein launchers, and everything a kernel decides for itself.
#pragma once
#include <cstdint>

#include "../../include/zafx.h"

// ---------------------------------------------------------------------------------
// The switches that enable a route (1: on).  Override with -D (tools/build_variant.sh, tools/variant_one.sh).
// ---------------------------------------------------------------------------------
// W = 4096, reference layout: 16-frame tiles in two bands of bins (k_stft_ft16b; buffer loads: 32-bit byte offsets inside a clip).
// Complex rows off the 128-byte grid: k_stft_ft16b writes every line in two parts far apart (1024 clips, two-sided, T = 217: 4.33 ms
// against 3.24 on the one-workgroup-per-tile kernel); the carry form k_stft_ft16bc (one band per workgroup) completes the lines:
// T = 217: 2.33 ms, T = 434 (hop 1024): 4.44 against 5.20.  One-sided output has half the stores to gain from and the form reads
// every sample twice: it wins at hop >= W / 2 only (T = 217: 1.89 against 1.96; hop 1024: 3.72 against 3.36 -> generic kernel).
// The float32 kinds write half lines either way and gain from k_stft_ft16b at every T (magnitude, T = 217: 1.33 against 1.67 ms).
#ifndef ZAFX_STFT_BAND
#define ZAFX_STFT_BAND 1
#endif
#ifndef ZAFX_STFT_BAND_CARRY
#define ZAFX_STFT_BAND_CARRY 1
#endif
// W = 8192, reference layout: 16-frame tiles in four classes of bins (k_stft_ft16q; 4-byte buffer loads: 32-bit byte offsets inside a clip).
// 1024 clips x 10 s, hop 4096, T = 112 (rows are whole lines): two-sided 2.19-2.29 ms against 2.77 on the one-workgroup-per-tile kernel, one-sided
// 1.68 against 1.99, |X| 1.60 against 1.84; T = 109: 3.3-4.3 against 3.04 two-sided (every line written in two parts by two workgroups: the
// generic kernel keeps those), 2.19 against 2.17 one-sided, 1.74 against 1.93 |X|
#ifndef ZAFX_STFT_QUAD
#define ZAFX_STFT_QUAD 1
#endif
// W = 256 ... 2048, complex rows off the 128-byte grid (the array itself only needs its 8-byte alignment): the carry form k_stft_ft16c
// writes whole lines anyway
#ifndef ZAFX_STFT_CARRY
#define ZAFX_STFT_CARRY 1
#endif
#ifndef ZAFX_STFT_CARRY_ALWAYS
#define ZAFX_STFT_CARRY_ALWAYS(log2n) ((log2n) == 9)   // W = 1024, two-sided: the carry form also on the line grid (863 / 864 frames: 1.90 ms against k_stft_ft16's 2.22; one-sided 1.31 against 1.21: not; W = 512, 256: 2.15 / 2.54 against 2.05 / 2.12: not)
#endif
// ISTFT, reference layout: W = 4096 at hop W / 2 on the two-class kernel k_istft_ft16d (every row read once; k_istft_ft16b reads 1.79 x the
// algorithmic bytes), W = 4096 at the other hops on the band form k_istft_ft16b, W = 8192 at hop W / 2 on the four-class kernel k_istft_ft8q
#ifndef ZAFX_ISTFT_DUO
#define ZAFX_ISTFT_DUO 1
#endif
#ifndef ZAFX_ISTFT_BAND
#define ZAFX_ISTFT_BAND 1
#endif
#ifndef ZAFX_ISTFT_QUAD
#define ZAFX_ISTFT_QUAD 1
#endif
// MDCT, reference layout: W = 4096 in two bands of bins (k_mdct_ft32b; its carry form k_mdct_ft32bc on rows off the 64-byte grid),
// W = 8192 in four (k_mdct_ft32q)
#ifndef ZAFX_MDCT_BAND
#define ZAFX_MDCT_BAND 1
#endif
#ifndef ZAFX_MDCT_BAND_CARRY
#define ZAFX_MDCT_BAND_CARRY 1
#endif
#ifndef ZAFX_MDCT_QUAD
#define ZAFX_MDCT_QUAD 1
#endif
// k_mdct_ft32 (W = 512 ... 2048) on rows that are not even whole 64-byte half lines (T % 16 != 0; odd T with 4-byte stores): the carry form --
// 1024 clips: T = 434 / 436 / 440 run 0.84 ms (4.3 TB/s) with it against 1.37 / 1.29 / 1.09 ms without.  At T % 16 == 0 (the benchmark's 432:
// odd rows start 64 bytes into a line and leave as two streamed half lines) the plain form is faster, 0.771 against 0.826 ms: the carry takes
// the registers of the resident window quadruples, worth 10 % on this LDS-bound kernel.
#ifndef ZAFX_MDCT_CARRY
#define ZAFX_MDCT_CARRY 1
#endif
// IMDCT at W = 8192 in the reference layout on the two-class kernel k_imdct_q
#ifndef ZAFX_IMDCT_QUAD
#define ZAFX_IMDCT_QUAD 1
#endif
// |X| / |X|^2 of an STFT plan at W = 2048 in the reference layout on k_mel2 (MODE 2 / 3)
#ifndef ZAFX_SPEC2
#define ZAFX_SPEC2 1
#endif
// mel / mfcc: k_mel2 at W = 2048 (the product of a tile under the transforms of the next), the fused two-band kernel k_mel_ft16b at W = 4096.
// k_mel2 is built for 16-frame tiles and 1024 threads: the two tile switches of k_mel are route conditions of it (kMel2Tile).
#ifndef ZAFX_MEL2
#define ZAFX_MEL2 1
#endif
#ifndef ZAFX_MEL_BAND
#define ZAFX_MEL_BAND 1
#endif
#ifndef ZAFX_MEL_THREADS
#define ZAFX_MEL_THREADS 1024
#endif
#ifndef ZAFX_MEL_FPB
#define ZAFX_MEL_FPB 16
#endif
// k_stft_ft16 at W = 2048: 1024 points as two radix-32 passes (its own twiddle table; run_stft_fat has the measurements)
#ifndef ZAFX_STFT_R32
#define ZAFX_STFT_R32 1
#endif

namespace zafx {

constexpr bool kMel2Tile = ZAFX_MEL_FPB == 16 && ZAFX_MEL_THREADS == 1024;

// What the conditions read of a call: the plan's geometry and tables, the call's counts, the two addresses.
struct RouteCall {
    int kind = 0, precision = 0;
    bool bluestein = false;
    int log2nf = 0, log2e = 0, layout = 0, spectrum = 0;
    int W = 0, H = 0, row_align = 0, n_filters = 0;
    // the plan's tables: pass / aux / radix-32 / sub / quad / band twiddles, the banded filterbank of k_melfb, the window on 16 bytes,
    // k_stft_ft16's claim word with the run-time split enabled, and the filterbank (and DCT) packed for k_mel2
    bool tw_pass = false, tw_aux = false, tw_r32 = false, tw_sub = false, tw_quad = false, tw_band = false, fbw = false, window16 = false,
         claim = false, mel2 = false;
    // the float32 window and the MDCT's folded one, and -- float64 plans -- the float64 window with the kind's tiled kernel (the
    // *_f64_tiled predicate of the equal-length float64 launchers, zafx_f64.hip)
    bool window = false, wfold = false, f64_tiled = false;
    int64_t n_clips = 0;
    int64_t n = 0;         // samples (center: sample frames; int16 PCM: frames) of a clip; unused by the inverses
    int T = 0;             // frames
    int64_t out_len = 0;   // the inverses: samples out
    uintptr_t in = 0, out = 0;
    int channels = 0, sample_bytes = 0;   // int16 / int32 PCM handed to zafx_execute_pcm (0: float samples)
};

// The answer: the route and the form of its kernel the launcher instantiates.
//   aligned  the buffer-load / wide-load form against the pointer form         carry    k_mdct_ft32's carry instantiation
//   vec      16-byte pieces of two adjacent frames (the inverse STFT kernels)  claimed  k_stft_ft16's tiles claimed at run time
//   pcm      the route has forms that read int16 in their own loads
template <class K>
struct Route {
    K k;
    bool aligned = false, vec = false, claimed = false, carry = false, pcm = false;
};

enum class StftRoute { Spec2, BandCarry, Band, Quad, FatCarry, Fat, Tf, Generic };
enum class IstftRoute { Duo, Band, Quad, Fat, Tf, Generic };
enum class MdctRoute { BandCarry, Band, Quad, Persistent, Generic };
enum class ImdctRoute { Quad, Generic };
enum class MelRoute { Mel2, Mel, Band, Wide };

// ---------------------------------------------------------------------------------
// route -> kernel name (what pl.ran and the planned names read), and the route's own name
// ---------------------------------------------------------------------------------
constexpr const char* kStftKernels[] = {"k_mel2", "k_stft_ft16bc", "k_stft_ft16b", "k_stft_ft16q", "k_stft_ft16c", "k_stft_ft16", "k_stft_tf", "k_stft"};
constexpr const char* kIstftKernels[] = {"k_istft_ft16d", "k_istft_ft16b", "k_istft_ft8q", "k_istft_ft16", "k_istft_ft16", "k_istft"};
constexpr const char* kMdctKernels[] = {"k_mdct_ft32bc", "k_mdct_ft32b", "k_mdct_ft32q", "k_mdct_ft32", "k_mdct"};
constexpr const char* kImdctKernels[] = {"k_imdct_q", "k_imdct"};
constexpr const char* kMelKernels[] = {"k_mel2", "k_mel", "k_mel_ft16b", "k_melfb"};
constexpr const char* kCqtKernel = "k_cqt";
constexpr const char* kCenterKernel = "k_center";
constexpr const char* kMaskfilterKernel = "k_maskfilter";
constexpr const char* kMaskfilterComplexKernel = "k_maskfilter_complex";                 // zafx_execute_masked_complex
constexpr const char* kMaskfilterComplexRaggedKernel = "k_maskfilter_complex_ragged";   // zafx_execute_masked_complex_ragged
constexpr const char* kMaskfilterStemsKernel ="k_maskfilter_stems";   // zafx_execute_masked_stems, whatever the stem count
constexpr int kMaskfilterMaxStems = 8;                                 // (ZAFX_MASKFILTER_MAX_STEMS: a carry of W/2 floats per stem in LDS)
constexpr const char* kernel_name(StftRoute r) { return kStftKernels[(int)r]; }
constexpr const char* kernel_name(IstftRoute r) { return kIstftKernels[(int)r]; }
constexpr const char* kernel_name(MdctRoute r) { return kMdctKernels[(int)r]; }
constexpr const char* kernel_name(ImdctRoute r) { return kImdctKernels[(int)r]; }
constexpr const char* kernel_name(MelRoute r) { return kMelKernels[(int)r]; }

constexpr const char* kStftRoutes[] = {"spec2", "band-carry", "band", "quad", "fat-carry", "fat", "tf", "generic"};
constexpr const char* kIstftRoutes[] = {"duo", "band", "quad", "fat", "tf", "generic"};
constexpr const char* kMdctRoutes[] = {"band-carry", "band", "quad", "persistent", "generic"};
constexpr const char* kImdctRoutes[] = {"quad", "generic"};
constexpr const char* kMelRoutes[] = {"mel2", "mel", "band", "wide"};
constexpr const char* route_name(StftRoute r) { return kStftRoutes[(int)r]; }
constexpr const char* route_name(IstftRoute r) { return kIstftRoutes[(int)r]; }
constexpr const char* route_name(MdctRoute r) { return kMdctRoutes[(int)r]; }
constexpr const char* route_name(ImdctRoute r) { return kImdctRoutes[(int)r]; }
constexpr const char* route_name(MelRoute r) { return kMelRoutes[(int)r]; }

// ---------------------------------------------------------------------------------
// the kernel families by window and layout (what `if constexpr` in the launchers and the planned names read)
// ---------------------------------------------------------------------------------
constexpr bool stft_use_fat(int log2n, int layout) {
    return layout == ZAFX_LAYOUT_FT && log2n >= 7 && log2n <= 10;   // one wavefront per frame
}
constexpr bool stft_use_tf(int log2n, int layout) {
    return layout == ZAFX_LAYOUT_TF && log2n >= 7 && log2n <= 10;   // one wavefront (or half of one) per frame
}
constexpr bool mdct_use_persistent(int log2nf, int /*layout*/) {
    return log2nf >= 7 && log2nf <= 9;   // either layout
}
// mel / mfcc plans that run as a spectrum kernel + k_melfb (or, W = 4096 with up to 256 filters, the fused two-band kernel) instead of k_mel
constexpr bool mel_wide(int log2nf, bool bluestein, int n_filters) { return log2nf >= 11 || bluestein || n_filters > 256; }

// The route a plan is built for (zafx_plan_kernel_name: does not change with the calls; what RAN is last_kernel).
constexpr StftRoute stft_planned_route(int log2n, int layout) {
    if (ZAFX_STFT_BAND && log2n == 11 && layout == ZAFX_LAYOUT_FT) return StftRoute::Band;
    if (ZAFX_STFT_QUAD && log2n == 12 && layout == ZAFX_LAYOUT_FT) return StftRoute::Quad;
    return stft_use_fat(log2n, layout) ? StftRoute::Fat : stft_use_tf(log2n, layout) ? StftRoute::Tf : StftRoute::Generic;
}
constexpr IstftRoute istft_planned_route(int log2n, int layout) {
    if (ZAFX_ISTFT_BAND && log2n == 11 && layout == ZAFX_LAYOUT_FT) return IstftRoute::Band;
    return stft_use_fat(log2n, layout) || stft_use_tf(log2n, layout) ? IstftRoute::Fat : IstftRoute::Generic;
}
constexpr MdctRoute mdct_planned_route(int log2nf, int layout) {
    if (ZAFX_MDCT_BAND && log2nf == 10 && layout == ZAFX_LAYOUT_FT) return MdctRoute::Band;
    if (ZAFX_MDCT_QUAD && log2nf == 11 && layout == ZAFX_LAYOUT_FT) return MdctRoute::Quad;
    return mdct_use_persistent(log2nf, layout) ? MdctRoute::Persistent : MdctRoute::Generic;
}
constexpr ImdctRoute imdct_planned_route() { return ImdctRoute::Generic; }
constexpr MelRoute mel_planned_route(int log2nf, int n_filters) {
    return n_filters > 256 ? MelRoute::Wide : log2nf == 11 ? MelRoute::Band : log2nf >= 12 ? MelRoute::Wide : MelRoute::Mel;
}

// ---------------------------------------------------------------------------------
// the conditions
// ---------------------------------------------------------------------------------
// Frames between the starts of consecutive rows of a plan's (F, T) array: T rounded up to row_align elements (reference-layout plans
// only; 0 / 1 = compact, the reference's own memory order).  row_pitch(plan, T) of zafx_internal.hpp forwards here.
constexpr int64_t row_pitch(int layout, int row_align, int64_t T) {
    const int64_t a = row_align;
    return (layout == ZAFX_LAYOUT_FT && a > 1) ? (T + a - 1) / a * a : T;
}
inline int64_t row_pitch(const RouteCall& c) { return row_pitch(c.layout, c.row_align, c.T); }

inline bool ft(const RouteCall& c) { return c.layout == ZAFX_LAYOUT_FT; }
inline int spec(const RouteCall& c) { return c.spectrum; }   // 0 two-sided, 1 one-sided, 2 |X|, 3 |X|^2: the launchers' SPEC
inline bool f32_pow2(const RouteCall& c) { return c.precision == ZAFX_PRECISION_F32 && !c.bluestein; }

// sample pairs as 8-byte loads
inline bool sample_pairs(const RouteCall& c) { return c.n % 2 == 0 && c.in % 8 == 0; }
// the STFT family's aligned form: every frame starts on a sample pair
inline bool stft_aligned(const RouteCall& c) { return (c.n % 2 == 0) && (c.H % 2 == 0) && (c.in % 8 == 0); }
// complex rows (float32 rows of the band kernels' |X|: half of them) that are whole 128-byte lines
inline bool rows_whole_lines(const RouteCall& c) { return row_pitch(c) % 16 == 0 && c.out % 128 == 0; }
// float32 rows that are not whole 64-byte half lines
inline bool rows_off_half_lines(const RouteCall& c) { return row_pitch(c) % 16 != 0 || c.out % 64 != 0; }
inline int tiles16(const RouteCall& c) { return (c.T + 15) / 16; }
inline int tiles32(const RouteCall& c) { return (c.T + 31) / 32; }
// a clip below 2^29 samples: 32-bit byte offsets inside one buffer descriptor
inline bool clip_below_2_29(const RouteCall& c) { return c.n < (1LL << 29); }
// ... and its frames with it (k_stft_ft16c's aligned form, the int16 STFT)
inline bool frames_addressable(const RouteCall& c) { return clip_below_2_29(c) && (long long)c.T * c.H < (1LL << 29); }
// W = 4096 on the two-band kernels (k_stft_ft16b, k_stft_ft16bc, k_mel_ft16b): the clip and the 16-frame halo of the tile they read ahead
inline bool band_addressable(const RouteCall& c) {
    return clip_below_2_29(c) && (long long)(c.T + 16) * c.H < (1LL << 29) && c.in % 4 == 0;
}
inline bool quad_addressable(const RouteCall& c) {
    return clip_below_2_29(c) && (long long)(c.T + 16) * c.H < (1LL << 28) && c.in % 4 == 0;
}
// a complex array whose row count fits the unit counters of the carry kernels
inline bool complex_out_countable(const RouteCall& c) { return c.out % 8 == 0 && c.n_clips * (long long)c.T < (1LL << 31); }

// |X| / |X|^2 at W = 2048 in the reference layout on k_mel2 (launch_spec2): the plan's part ...
inline bool spec2_geometry(const RouteCall& c) {
    return ZAFX_SPEC2 && c.log2nf == 10 && c.log2e == 4 && ft(c) && kMel2Tile && c.tw_pass && c.tw_aux &&
           (c.spectrum == ZAFX_SPECTRUM_MAGNITUDE || c.spectrum == ZAFX_SPECTRUM_POWER);
}
// ... and the call's: the clip and the tile count (a ragged batch asks the same of every clip and of its own tiles, ragged_route)
inline bool spec2_usable(const RouteCall& c) { return spec2_geometry(c) && clip_below_2_29(c) && (long long)tiles16(c) * c.n_clips < (1LL << 31); }

// forward STFT (float32, power-of-two window): launch_stft
inline Route<StftRoute> stft_route(const RouteCall& c) {
    using R = Route<StftRoute>;
    const bool aligned = stft_aligned(c);
    const int SPEC = spec(c), LOG2N = c.log2nf;
    if (spec2_usable(c)) {
        R r{StftRoute::Spec2};
        r.aligned = aligned, r.pcm = true;
        return r;
    }
    if (ZAFX_STFT_BAND && LOG2N == 11 && ft(c)) {
        const bool whole = rows_whole_lines(c);
        const bool fits = c.tw_sub && (long long)c.n_clips * tiles16(c) < (1LL << 30) && band_addressable(c);
        if (SPEC < 2 && ZAFX_STFT_BAND_CARRY) {
            if (!whole && fits && (SPEC == 0 || 2 * c.H >= c.W) && complex_out_countable(c)) {
                R r{StftRoute::BandCarry};
                r.aligned = aligned;
                return r;
            }
        }
        if ((SPEC >= 2 || whole) && c.tw_sub && (long long)c.n_clips * tiles16(c) < (1LL << 31) && band_addressable(c)) {
            R r{StftRoute::Band};
            r.aligned = aligned;
            return r;
        }
    }
    if (ZAFX_STFT_QUAD && LOG2N == 12 && ft(c)) {
        if ((SPEC != 0 || rows_whole_lines(c)) && c.tw_sub && c.tw_quad && (long long)c.n_clips * tiles16(c) < (1LL << 31) && quad_addressable(c))
            return R{StftRoute::Quad};
    }
    if (stft_use_fat(LOG2N, c.layout)) {
        if (SPEC < 2 && ZAFX_STFT_CARRY) {
            if (((SPEC == 0 && ZAFX_STFT_CARRY_ALWAYS(LOG2N)) || !rows_whole_lines(c)) && complex_out_countable(c)) {
                R r{StftRoute::FatCarry};
                r.aligned = aligned && frames_addressable(c);
                r.pcm = LOG2N == 10 && r.aligned;
                return r;
            }
        }
        R r{StftRoute::Fat};
        r.aligned = aligned;
        r.pcm = LOG2N == 10 && SPEC < 2;
        r.claimed = SPEC < 2 && c.claim && rows_whole_lines(c);   // (float samples only: the launcher knows the thread's PCM mode)
        return r;
    }
    R r{stft_use_tf(LOG2N, c.layout) ? StftRoute::Tf : StftRoute::Generic};
    r.aligned = r.k == StftRoute::Tf && aligned;
    return r;
}

// ISTFT: the spectrum of one clip -- counted as `rows` rows, one-sided too -- behind signed 32-bit byte offsets
inline bool spectrum_addressable(const RouteCall& c, int rows) { return (long long)rows * row_pitch(c) * 8 < (1LL << 31); }
// 16-byte row pieces of two adjacent frames
inline bool spectrum_pairs(const RouteCall& c) { return row_pitch(c) % 2 == 0 && c.in % 16 == 0; }

inline Route<IstftRoute> istft_route(const RouteCall& c) {
    using R = Route<IstftRoute>;
    const int LOG2N = c.log2nf;
    const int T = c.T;
    if (ZAFX_ISTFT_DUO && LOG2N == 11 && ft(c)) {
        // W = 4096, hop = W / 2: the two-class kernel (16-byte stores into the clip's samples)
        if (c.tw_sub && c.tw_aux && c.H == 2048 && c.in % 8 == 0 && c.out % 16 == 0 && spectrum_addressable(c, 4096) &&
            c.n_clips * (((long long)T + 15) / 16 + 1) < (1LL << 30)) {
            R r{IstftRoute::Duo};
            r.vec = spectrum_pairs(c);
            return r;
        }
    }
    if (ZAFX_ISTFT_BAND && LOG2N == 11 && ft(c)) {
        // W = 4096: the band form wants a hop that is a multiple of 4 (a sample keeps its residue mod 4 from frame to frame), at least 512
        // (ceil(W / H) - 1 <= 7 halo frames; the carry fits LDS)
        if (c.tw_sub && c.H % 4 == 0 && c.H >= 512 && c.H <= 4096 && c.in % 8 == 0 && spectrum_addressable(c, 4096) &&
            2LL * c.n_clips * ((T + 15) / 16) < (1LL << 30)) {
            R r{IstftRoute::Band};
            r.vec = spectrum_pairs(c);
            return r;
        }
    }
    if (ZAFX_ISTFT_QUAD && LOG2N == 12 && ft(c)) {
        // W = 8192, hop = W / 2: the four-class kernel (16-byte stores into the clip's samples)
        if (c.tw_sub && c.tw_quad && c.H == 4096 && c.in % 8 == 0 && c.out % 16 == 0 && spectrum_addressable(c, 8192) &&
            c.n_clips * (((long long)T + 7) / 8 + 1) < (1LL << 30)) {
            R r{IstftRoute::Quad};
            r.vec = spectrum_pairs(c);
            return r;
        }
    }
    if (stft_use_fat(LOG2N, c.layout)) {
        // the carry kernel addresses a clip through one buffer descriptor
        if (spectrum_addressable(c, 2 << LOG2N)) {
            R r{IstftRoute::Fat};
            r.vec = LOG2N >= 8 && c.in % 8 == 0;   // 16-byte gathers (two adjacent frames per lane) at any 8-byte offset
            return r;
        }
    } else if (stft_use_tf(LOG2N, c.layout)) {
        return R{IstftRoute::Tf};
    }
    return R{IstftRoute::Generic};
}

// MDCT: 16-byte buffer loads -- clips of a multiple of four samples on 16 bytes, 32-bit byte offsets inside a clip
inline bool mdct_aligned(const RouteCall& c) { return c.n % 4 == 0 && c.in % 16 == 0 && c.n < (1LL << 28); }

inline Route<MdctRoute> mdct_route(const RouteCall& c) {
    using R = Route<MdctRoute>;
    const int LOG2NF = c.log2nf;
    if (ZAFX_MDCT_BAND && ZAFX_MDCT_BAND_CARRY && LOG2NF == 10 && ft(c)) {
        // rows that are not whole 64-byte half lines: the carry form (one band per workgroup)
        if (c.tw_sub && c.tw_band && mdct_aligned(c) && rows_off_half_lines(c) && c.out % 4 == 0 && 2LL * c.n_clips * tiles32(c) < (1LL << 30) &&
            (long long)c.n_clips * 2048 * row_pitch(c) < (1LL << 40))
            return R{MdctRoute::BandCarry};
    }
    if (ZAFX_MDCT_BAND && LOG2NF == 10 && ft(c)) {
        if (c.tw_sub && c.tw_band && mdct_aligned(c) && (long long)c.n_clips * tiles32(c) < (1LL << 31)) return R{MdctRoute::Band};
    }
    if (ZAFX_MDCT_QUAD && LOG2NF == 11 && ft(c)) {
        // 4-byte buffer loads with 33 frames of halo behind 32-bit byte offsets
        if (c.tw_sub && c.tw_quad && c.n < (1LL << 28) && (long long)(c.T + 33) * 4096 < (1LL << 28) && c.in % 4 == 0 && c.out % 4 == 0 &&
            (long long)c.n_clips * tiles32(c) < (1LL << 31)) {
            R r{MdctRoute::Quad};
            r.aligned = sample_pairs(c);
            return r;
        }
    }
    if (mdct_use_persistent(LOG2NF, c.layout)) {
        R r{MdctRoute::Persistent};
        r.aligned = mdct_aligned(c);
        r.pcm = LOG2NF == 9 && ft(c);
        r.carry = ft(c) && ZAFX_MDCT_CARRY && r.aligned && rows_off_half_lines(c) && (long long)tiles32(c) * c.n_clips < (1LL << 31);
        return r;
    }
    return R{MdctRoute::Generic};
}

// IMDCT at W = 8192: four frames per 16-byte piece (a row pitch that is a multiple of 4), 32-bit byte offsets inside a clip's coefficients
inline Route<ImdctRoute> imdct_route(const RouteCall& c) {
    using R = Route<ImdctRoute>;
    if (ZAFX_IMDCT_QUAD && c.log2nf == 11 && ft(c)) {
        const int64_t TP = row_pitch(c);
        if (c.tw_sub && c.tw_quad && TP % 4 == 0 && c.in % 16 == 0 && c.window16 && (long long)4096 * TP * 4 < (1LL << 31) &&
            c.n_clips * (((long long)c.T + 15) / 16 + 1) < (1LL << 30))
            return R{ImdctRoute::Quad};
    }
    return R{ImdctRoute::Generic};
}

// mel / mfcc.  The aligned form of k_mel / k_mel2 addresses a clip through one buffer descriptor: clips below 2^29 samples.
inline bool mel_aligned(const RouteCall& c) { return stft_aligned(c) && clip_below_2_29(c); }
// W = 4096: the fused two-band kernel k_mel_ft16b.  false: the spectrum kernel + k_melfb (clips too long for 32-bit byte offsets, unaligned base)
inline bool mel_band_usable(const RouteCall& c) {
    return c.log2nf == 11 && c.tw_sub && c.fbw && c.n_filters <= 256 && band_addressable(c) && (long long)c.n_clips * tiles16(c) < (1LL << 31);
}
inline Route<MelRoute> mel_route(const RouteCall& c) {
    using R = Route<MelRoute>;
    if (mel_wide(c.log2nf, c.bluestein, c.n_filters)) {
        if (ZAFX_MEL_BAND && mel_band_usable(c)) {
            R r{MelRoute::Band};
            r.aligned = stft_aligned(c);
            return r;
        }
        return R{MelRoute::Wide};
    }
    R r{ZAFX_MEL2 && c.log2nf == 10 && c.log2e == 4 && kMel2Tile && c.mel2 ? MelRoute::Mel2 : MelRoute::Mel};   // (run_mel picks between the two)
    r.aligned = mel_aligned(c);
    r.pcm = r.k == MelRoute::Mel2;
    return r;
}

// int16 PCM (one or two channels) read by the kernels' own loads (zafx_execute_pcm); everything else converts into a float32 staging array first
constexpr bool pcm_int16(int channels, int sample_bytes) { return sample_bytes == 2 && (channels == 1 || channels == 2); }
inline bool pcm_int16(const RouteCall& c) { return pcm_int16(c.channels, c.sample_bytes); }
// ... on k_mel2: mel / mfcc and |X| / |X|^2 at W = 2048 (the caller checks the array's 8-byte alignment)
inline bool pcm_direct_ok(const RouteCall& c) {
    if (!pcm_int16(c) || c.precision != ZAFX_PRECISION_F32 || c.bluestein) return false;
    if (c.log2nf != 10 || c.log2e != 4 || !kMel2Tile || !clip_below_2_29(c)) return false;
    if (c.kind == ZAFX_MEL || c.kind == ZAFX_MFCC) return ZAFX_MEL2 && !mel_wide(c.log2nf, c.bluestein, c.n_filters) && c.mel2;
    if (c.kind == ZAFX_STFT) return ZAFX_SPEC2 && ft(c) && (c.spectrum == ZAFX_SPECTRUM_MAGNITUDE || c.spectrum == ZAFX_SPECTRUM_POWER);
    return false;
}
// ... on the complex STFT at W = 2048 in the reference layout (k_stft_ft16 / k_stft_ft16c): even clip length and hop, everything inside the
// 32-bit offsets of one descriptor
inline bool stft_pcm_direct_ok(const RouteCall& c) {
    return pcm_int16(c) && c.kind == ZAFX_STFT && f32_pow2(c) && c.log2nf == 10 && ft(c) && c.spectrum <= ZAFX_SPECTRUM_ONE_SIDED && stft_aligned(c) &&
           frames_addressable(c);
}
// ... on k_mdct_ft32: W = 2048, reference layout, clips of a multiple of four frames
inline bool mdct_pcm_direct_ok(const RouteCall& c) {
    return pcm_int16(c) && c.kind == ZAFX_MDCT && f32_pow2(c) && c.log2nf == 9 && ft(c) && mdct_aligned(c);
}

// refusals: a clip is addressed through one buffer descriptor with 32-bit byte offsets
inline bool cqt_clip_refused(const RouteCall& c) { return c.n >= (1LL << 29); }
inline bool center_clip_refused(const RouteCall& c) { return c.n >= (1LL << 28); }   // (sample frames)
// ---------------------------------------------------------------------------------
// The fused STFT -> mask -> ISTFT family: four kinds of mask, each with an equal-length and a ragged entry point (zafx_execute_masked*).
// What the refusals of a kind read stands in one record; zafx_capi.cpp (kMaskedForms) and zafx/core.py (_MaskedForm) hold the rest of a kind.
// The strings and the order of the tests are those the per-kind functions had (profiles/maskfilter_forms_notes.md: the irregularities kept).
// ---------------------------------------------------------------------------------
struct MaskfilterForm {
    const char* wrong_kind;        // what a plan of another kind is told ...
    bool equal_asks_kind;          // ... by the equal-length refusal too (stems: no -- its entry point has asked in its own words)
    const char* wrong_layout;      // masks in ZAFX_LAYOUT_TF only (null: ZAFX_LAYOUT_FT too)
    int64_t count_min, count_max;  // the count argument -- n_stems, mask_channels -- ...
    const char* wrong_count;       // ... and what a value outside is told (null: the kind has no count)
    int64_t max_units;             // clips of this many samples (stereo: sample frames) and more are refused ...
    int64_t halved_at;             // ... of half as many at this count (0: at none)
    const char* too_long[2];       // the equal-length call's refusal of such a clip, [1]: at the halved bound
    const char* clip_too_long[2];  // the ragged call's (the caller appends the clip's index)
    int mask_bytes;                // of a mask element
    bool count_in_descriptor;      // the count's masks of a frame lie behind ONE buffer descriptor (stems: one descriptor per stem)
    constexpr int halved(int64_t count) const { return halved_at != 0 && count == halved_at; }
    constexpr int64_t bound(int64_t count) const { return max_units >> halved(count); }
};
// k_maskfilter: one real mask in the plan's layout.  Its entry points ask the kind in their own words and leave the equal-length bound to the
// launcher (maskfilter_clip_refused); the ragged one names the clip in front (check_clips_below_2_28, zafx_capi.cpp): clip_too_long is not used.
constexpr MaskfilterForm kMaskfilterReal = {
    "ZAFX_MASKFILTER and ZAFX_MASKFILTER_REST plans only (zafx_execute_ragged takes the forward kinds)", false, nullptr, 0, 0, nullptr, 1LL << 28, 0,
    {"mask filter: clips of 2^28 samples and more are not supported", nullptr}, {nullptr, nullptr}, 4, false};
// k_maskfilter_stems: masks in ZAFX_LAYOUT_TF only (k_maskfilter's FT stage and eight carries do not fit LDS at W = 2048), 1 .. 8 stems, and the
// clip bound of the one-mask kind -- a descriptor per (clip, stem) addresses one mask, as there -- in that kind's words.
constexpr MaskfilterForm kMaskfilterStems = {
    "mask filter stems: ZAFX_MASKFILTER and ZAFX_MASKFILTER_REST plans only", false,
    "mask filter stems: masks in ZAFX_LAYOUT_TF only (create the plan with layout = ZAFX_LAYOUT_TF)", 1, kMaskfilterMaxStems,
    "mask filter stems: n_stems must be in 1 .. 8 (ZAFX_MASKFILTER_MAX_STEMS)", 1LL << 28, 0,
    {kMaskfilterReal.too_long[0], nullptr}, {"mask filter stems: a clip has 2^28 samples or more (not supported)", nullptr}, 4, false};
// k_maskfilter_c: complex64 masks in ZAFX_LAYOUT_TF only (the FT stage in LDS would double: 148 KB at W = 2048 beside the frames), and clips
// below 2^27 samples: a clip's mask -- 8 bytes a bin, T (W/2 + 1) bins -- lies behind one buffer descriptor with signed 32-bit byte offsets.
constexpr MaskfilterForm kMaskfilterComplex = {
    "complex mask filter: ZAFX_MASKFILTER and ZAFX_MASKFILTER_REST plans only", true,
    "complex mask filter: masks in ZAFX_LAYOUT_TF only (create the plan with layout = ZAFX_LAYOUT_TF)", 0, 0, nullptr, 1LL << 27, 0,
    {"complex mask filter: clips of 2^27 samples and more are not supported", nullptr},
    {"complex mask filter: a clip has 2^27 samples or more (not supported)", nullptr}, 8, false};
// k_maskfilter_stereo: interleaved stereo clips under one real mask for both channels (mask_channels 1) or one per channel (2), masks in
// ZAFX_LAYOUT_TF only (the kernel is k_center's walk: no FT stage in its LDS).  The samples lie behind one descriptor of 8 N bytes: N < 2^28
// sample frames; two masks per frame are 8 T (W/2 + 1) bytes -- the complex kind's arithmetic --: N < 2^27 then.
constexpr MaskfilterForm kMaskfilterStereo = {
    "stereo mask filter: ZAFX_MASKFILTER and ZAFX_MASKFILTER_REST plans only", true,
    "stereo mask filter: masks in ZAFX_LAYOUT_TF only (create the plan with layout = ZAFX_LAYOUT_TF)", 1, 2,
    "stereo mask filter: mask_channels must be 1 (one mask for both channels) or 2 (one per channel)", 1LL << 28, 2,
    {"stereo mask filter: clips of 2^28 sample frames and more are not supported",
     "stereo mask filter: with a mask per channel clips of 2^27 sample frames and more are not supported"},
    {"stereo mask filter: a clip has 2^28 sample frames or more (not supported)",
     "stereo mask filter: with a mask per channel a clip has 2^27 sample frames or more (not supported)"}, 4, true};

// bytes of the compact TF mask(s) behind one descriptor of a clip of n samples (sample frames): T frames of W/2 + 1 bins
constexpr int64_t maskfilter_mask_bytes(const MaskfilterForm& f, int64_t n, int W, int64_t count) {
    return ((n + W / 2 - 1) / (W / 2) + 1) * (f.count_in_descriptor ? count : 1) * (W / 2 + 1) * f.mask_bytes;
}
constexpr bool maskfilter_masks_addressable(const MaskfilterForm& f) {
    for (int W = 256; W <= 2048; W *= 2)
        for (int64_t count = f.count_min; count <= f.count_max; ++count)
            if (maskfilter_mask_bytes(f, f.bound(count) - 1, W, count) >= (1LL << 31)) return false;
    return true;
}
static_assert(maskfilter_masks_addressable(kMaskfilterReal) && maskfilter_masks_addressable(kMaskfilterStems) &&
                  maskfilter_masks_addressable(kMaskfilterComplex) && maskfilter_masks_addressable(kMaskfilterStereo),
              "mask filter, every window, kind and count: the mask(s) of the longest clip taken stay behind signed 32-bit byte offsets");

// The equal-length call: reads kind (where the form asks it), layout and n.  nullptr: the call is taken.
inline const char* maskfilter_form_refusal(const MaskfilterForm& f, const RouteCall& c, int64_t count, bool ask_kind) {
    if (ask_kind && c.kind != ZAFX_MASKFILTER && c.kind != ZAFX_MASKFILTER_REST) return f.wrong_kind;
    if (f.wrong_layout && c.layout != ZAFX_LAYOUT_TF) return f.wrong_layout;
    if (f.wrong_count && (count < f.count_min || count > f.count_max)) return f.wrong_count;
    if (c.n >= f.bound(count)) return f.too_long[f.halved(count)];
    return nullptr;
}
inline const char* maskfilter_form_refusal(const MaskfilterForm& f, const RouteCall& c, int64_t count) { return maskfilter_form_refusal(f, c, count, f.equal_asks_kind); }
// The ragged call: the kind, the layout and the count as above, then every clip's length against the bound, before anything is read.
// nullptr: the call is taken; otherwise *clip is the index of the clip refused, or -1 where the refusal is none of a clip's.
inline const char* maskfilter_form_ragged_refusal(const MaskfilterForm& f, int kind, int layout, int64_t count, const int64_t* lengths, int64_t n_clips, int64_t* clip) {
    *clip = -1;
    RouteCall c;
    c.kind = kind, c.layout = layout;
    if (const char* why = maskfilter_form_refusal(f, c, count, true)) return why;
    for (int64_t i = 0; i < n_clips; ++i)
        if (lengths[i] >= f.bound(count)) {
            *clip = i;
            return f.clip_too_long[f.halved(count)];
        }
    return nullptr;
}

// The names the launchers, the entry points and tests/host_emu reach for: each a call onto its kind's record.
inline bool maskfilter_clip_refused(const RouteCall& c) { return c.n >= kMaskfilterReal.bound(0); }   // (samples; the clip's mask then stays below 2^31 bytes)
inline const char* maskfilter_stems_refusal(const RouteCall& c, int64_t n_stems) { return maskfilter_form_refusal(kMaskfilterStems, c, n_stems); }
inline const char* maskfilter_stems_ragged_refusal(int kind, int layout, int64_t n_stems, const int64_t* lengths, int64_t n_clips, int64_t* clip) {
    return maskfilter_form_ragged_refusal(kMaskfilterStems, kind, layout, n_stems, lengths, n_clips, clip);
}
constexpr int64_t kMaskfilterComplexMaxSamples = kMaskfilterComplex.max_units;
constexpr int64_t maskfilter_complex_mask_bytes(int64_t n, int W) { return maskfilter_mask_bytes(kMaskfilterComplex, n, W, 0); }
inline bool maskfilter_complex_clip_refused(const RouteCall& c) { return c.n >= kMaskfilterComplex.bound(0); }
inline const char* maskfilter_complex_refusal(const RouteCall& c) { return maskfilter_form_refusal(kMaskfilterComplex, c, 0); }
inline const char* maskfilter_complex_ragged_refusal(int kind, int layout, const int64_t* lengths, int64_t n_clips, int64_t* clip) {
    return maskfilter_form_ragged_refusal(kMaskfilterComplex, kind, layout, 0, lengths, n_clips, clip);
}
constexpr int64_t maskfilter_stereo_max_frames(int64_t mask_channels) { return kMaskfilterStereo.bound(mask_channels); }
constexpr int64_t maskfilter_stereo_mask_bytes(int64_t n, int W, int64_t mask_channels) { return maskfilter_mask_bytes(kMaskfilterStereo, n, W, mask_channels); }
constexpr const char* kMaskfilterStereoKernel = "k_maskfilter_stereo";                 // zafx_execute_masked_stereo
constexpr const char* kMaskfilterStereoRaggedKernel = "k_maskfilter_stereo_ragged";   // zafx_execute_masked_stereo_ragged
inline bool maskfilter_stereo_clip_refused(const RouteCall& c, int64_t mask_channels) { return c.n >= kMaskfilterStereo.bound(mask_channels); }
inline const char* maskfilter_stereo_refusal(const RouteCall& c, int64_t mask_channels) { return maskfilter_form_refusal(kMaskfilterStereo, c, mask_channels); }
inline const char* maskfilter_stereo_ragged_refusal(int kind, int layout, int64_t mask_channels, const int64_t* lengths, int64_t n_clips, int64_t* clip) {
    return maskfilter_form_ragged_refusal(kMaskfilterStereo, kind, layout, mask_channels, lengths, n_clips, clip);
}

// The PCM forms (zafx_execute_masked_pcm, zafx_execute_masked_pcm_ragged; zafx_maskfilter_pcm.hip): int16 samples in, int16 or float32 samples
// out, on k_maskfilter_pcm (n_channels 1) and k_maskfilter_stereo_pcm (2).  The stereo form refuses what the float stereo kind refuses, from
// that kind's record.  The mono form has the real kind's bound in the real kind's words and masks in ZAFX_LAYOUT_TF only (the FT stage of
// k_maskfilter has no PCM form).
constexpr const char* kMaskfilterPcmKernel = "k_maskfilter_pcm";
constexpr const char* kMaskfilterPcmRaggedKernel = "k_maskfilter_pcm_ragged";
constexpr const char* kMaskfilterStereoPcmKernel = "k_maskfilter_stereo_pcm";
constexpr const char* kMaskfilterStereoPcmRaggedKernel = "k_maskfilter_stereo_pcm_ragged";
constexpr MaskfilterForm kMaskfilterPcmMono = {
    "PCM mask filter: ZAFX_MASKFILTER and ZAFX_MASKFILTER_REST plans only", true,
    "PCM mask filter: masks in ZAFX_LAYOUT_TF only (create the plan with layout = ZAFX_LAYOUT_TF)", 0, 0, nullptr, kMaskfilterReal.max_units, 0,
    {kMaskfilterReal.too_long[0], nullptr}, {"PCM mask filter: a clip has 2^28 samples or more (not supported)", nullptr}, 4, false};
static_assert(maskfilter_masks_addressable(kMaskfilterPcmMono), "PCM mask filter: the mask of the longest clip taken stays behind signed 32-bit byte offsets");
constexpr const MaskfilterForm& maskfilter_pcm_form(int n_channels) { return n_channels == 2 ? kMaskfilterStereo : kMaskfilterPcmMono; }
// n_channels 1 (mask_channels 1 then) or 2 (mask_channels 1 or 2, which the stereo record asks again); nullptr: taken
inline const char* maskfilter_pcm_channels_refusal(int64_t n_channels, int64_t mask_channels) {
    if (n_channels != 1 && n_channels != 2) return "PCM mask filter: n_channels must be 1 (mono) or 2 (interleaved stereo)";
    if (mask_channels != 1 && mask_channels != 2) return "PCM mask filter: mask_channels must be 1 or 2";
    if (n_channels == 1 && mask_channels != 1) return "PCM mask filter: mask_channels must be 1 with one channel (a mask per channel takes n_channels 2)";
    return nullptr;
}
inline const char* maskfilter_pcm_out_refusal(int64_t out_sample_bytes) {
    return out_sample_bytes == 2 || out_sample_bytes == 4 ? nullptr : "PCM mask filter: out_sample_bytes must be 2 (int16) or 4 (float32)";
}
// The arrays: int16 samples on the sample-frame grid (2 bytes mono, 4 stereo), float32 samples and masks on 4 bytes.  A stereo array off its
// grid would turn every dword of the kernel into a misaligned one; it is refused, not rounded.
inline const char* maskfilter_pcm_alignment_refusal(uintptr_t in, uintptr_t mask, uintptr_t out, int n_channels, int out_sample_bytes) {
    if (in % (uintptr_t)(2 * n_channels) != 0)
        return n_channels == 2 ? "PCM mask filter: d_pcm must be 4-byte aligned (stereo int16: the sample-frame grid)" : "PCM mask filter: d_pcm must be 2-byte aligned";
    if (mask % 4 != 0) return "PCM mask filter: d_mask must be 4-byte aligned";
    if (out % (uintptr_t)(out_sample_bytes == 2 ? 2 * n_channels : 4) != 0)
        return out_sample_bytes == 4 ? "PCM mask filter: d_out must be 4-byte aligned (float32)"
               : n_channels == 2     ? "PCM mask filter: d_out must be 4-byte aligned (stereo int16: the sample-frame grid)"
                                     : "PCM mask filter: d_out must be 2-byte aligned";
    return nullptr;
}
// What the sample types add to a call, in the order the entry points ask it: the channels, the output type, the arrays' grids.  nullptr: the
// call goes on to the refusals of maskfilter_pcm_form(n_channels) with count = mask_channels (stereo) or 0 (mono).
inline const char* maskfilter_pcm_call_refusal(int64_t n_channels, int64_t mask_channels, int64_t out_sample_bytes, uintptr_t in, uintptr_t mask, uintptr_t out) {
    if (const char* why = maskfilter_pcm_channels_refusal(n_channels, mask_channels)) return why;
    if (const char* why = maskfilter_pcm_out_refusal(out_sample_bytes)) return why;
    return maskfilter_pcm_alignment_refusal(in, mask, out, (int)n_channels, (int)out_sample_bytes);
}

// ---------------------------------------------------------------------------------
// ragged batches: clips of different lengths in one call (zafx_execute_ragged, zafx_execute_ragged_pcm, zafx_execute_imdct_ragged,
// zafx_execute_istft_ragged).  The tests run in the order, and with the inequalities, the entry points had inline
// (profiles/routes_notes.md lists the ones that look inconsistent).
// ---------------------------------------------------------------------------------
// frames per tile of the RAGGED kernel forms: what the host's tables count (each launcher static_asserts its own against the kernel's)
constexpr int kStftRaggedTile = 16;                           // k_stft_ft16, k_mel2
constexpr int kMdctRaggedTile = 32;                           // k_mdct_ft32
constexpr int kStft64RaggedTile = 8, kMd64RaggedTile = 16;    // k_stft_ft8_f64; k_mdct_ft16_f64, k_mel_ft8_f64
constexpr int kImdctRaggedTile = 32, kIstftRaggedTile = 16;   // k_imdct, k_istft_ft16

enum class RaggedRoute { MdctNative, F64Native, StftNative, MelNative, PerClip, PcmNotTaken };
// the RAGGED forms' names (what pl.ran reads after a native launch)
enum class RaggedKernel { Stft, Mel2, Mdct, Istft, Imdct, Stft64, Mdct64, Mel64 };
constexpr const char* kRaggedKernels[] = {"k_stft_ft16_ragged", "k_mel2_ragged",          "k_mdct_ft32_ragged",     "k_istft_ragged",
                                          "k_imdct_ragged",     "k_stft_ft8_f64_ragged", "k_mdct_ft16_f64_ragged", "k_mel_ft8_f64_ragged"};
constexpr const char* kernel_name(RaggedKernel k) { return kRaggedKernels[(int)k]; }

// bytes of an element of a forward plan's output: complex for the two complex kinds of the STFT
constexpr int64_t out_elem_bytes(int kind, int precision, int spectrum) {
    return (precision == ZAFX_PRECISION_F64 ? 8 : 4) * (kind == ZAFX_STFT && spectrum < ZAFX_SPECTRUM_MAGNITUDE ? 2 : 1);
}
// What the kernels ask of the clips of a batch, one field per question: add() takes one clip -- its offset and length in the input array,
// its frames, the pitch of its rows and the bytes of an output element.
struct RaggedBatch {
    bool whole_lines = true;                       // every block's rows are whole 128-byte lines, at a pitch below 2^31
    bool below_2_29 = true, below_2_28 = true;     // every clip's length
    bool offsets_even = true, lengths_even = true;
    bool quads = true;                             // every offset and length a multiple of 4
    int64_t tiles8 = 0, tiles16 = 0, tiles32 = 0;  // the batch's tiles of 8 / 16 / 32 frames (whole_lines: every frame count fits the record's int)
    int64_t n_clips = 0;
    void add(int64_t offset, int64_t length, int64_t frames, int64_t pitch, int64_t elem_bytes) {
        whole_lines = whole_lines && (pitch * elem_bytes) % 128 == 0 && pitch < INT32_MAX;
        below_2_29 = below_2_29 && length < (1LL << 29);
        below_2_28 = below_2_28 && length < (1LL << 28);
        offsets_even = offsets_even && offset % 2 == 0;
        lengths_even = lengths_even && length % 2 == 0;
        quads = quads && offset % 4 == 0 && length % 4 == 0;
        tiles8 += (frames + 7) / 8, tiles16 += (frames + 15) / 16, tiles32 += (frames + 31) / 32;
        ++n_clips;
    }
    // "batch too large for one launch": checked after every clip, so the first clip that reaches the bound is the one reported
    bool too_large() const { return tiles16 >= (1LL << 31); }
};

// The plans that have a RAGGED kernel form (RouteCall: the plan's fields; the launchers' own guards ask the same functions).
// |X| / |X|^2 at W = 2048 on k_mel2: spec2_usable's geometry
inline bool spec2_ragged(const RouteCall& c) { return c.kind == ZAFX_STFT && f32_pow2(c) && spec2_geometry(c); }
// k_stft_ft16: W = 256 ... 2048 in the reference layout (W = 1024 two-sided too, where the equal-length route prefers the carry form)
inline bool stft_ragged_native(const RouteCall& c) {
    if (spec2_ragged(c)) return true;
    return c.kind == ZAFX_STFT && f32_pow2(c) && stft_use_fat(c.log2nf, c.layout) && c.tw_pass && c.tw_aux && (c.log2nf != 10 || !ZAFX_STFT_R32 || c.tw_r32);
}
// k_mel2: mel / mfcc of the geometries mel_route sends there, and the STFT plans of spec2_ragged
inline bool mel_ragged_native(const RouteCall& c) {
    if (c.kind == ZAFX_STFT) return spec2_ragged(c);
    if (c.kind != ZAFX_MEL && c.kind != ZAFX_MFCC) return false;
    if (!ZAFX_MEL2 || !f32_pow2(c) || !ft(c) || mel_wide(c.log2nf, c.bluestein, c.n_filters)) return false;
    return c.log2nf == 10 && c.log2e == 4 && kMel2Tile && c.mel2;
}
// k_mdct_ft32: W = 512, 1024, 2048 in the reference layout
inline bool mdct_ragged_native(const RouteCall& c) {
    return c.kind == ZAFX_MDCT && f32_pow2(c) && ft(c) && mdct_use_persistent(c.log2nf, c.layout) && c.wfold && c.tw_pass && c.tw_aux;
}
// k_imdct: W = 512, 1024, 2048 in the reference layout
inline bool imdct_ragged_native(const RouteCall& c) {
    return c.kind == ZAFX_IMDCT && f32_pow2(c) && ft(c) && mdct_use_persistent(c.log2nf, c.layout) && c.window && c.tw_pass && c.tw_aux;
}
// k_istft_ft16: W = 256 ... 2048 in the reference layout, any hop whose halo stays inside one tile
inline bool istft_ragged_native(const RouteCall& c) {
    return c.kind == ZAFX_ISTFT && f32_pow2(c) && stft_use_fat(c.log2nf, c.layout) && c.tw_pass && c.tw_aux && c.H >= 1 &&
           (c.W + c.H - 1) / c.H - 1 < kIstftRaggedTile;
}

// zafx_execute_ragged_pcm: the int16 mode its one launch runs in (1 mono, 2 stereo; 0: the batch converts to float32 first).
// pcm_native: ZAFX_RAGGED_PCM_NATIVE
inline int ragged_pcm_mode(int channels, int sample_bytes, bool pcm_native) { return pcm_int16(channels, sample_bytes) && pcm_native ? channels : 0; }

// The launch of a forward batch, the `aligned` argument of a native one and the frames per tile its table is built for.
struct RaggedAnswer { RaggedRoute k; bool aligned = false; int tile_frames = 0; };
// pcm: ragged_pcm_mode's answer (0: float samples) -- an int16 batch runs a native launch or none (PcmNotTaken; there is no per-clip path
// for integers).  mdct_native, f64_native: ZAFX_RAGGED_MDCT_NATIVE, ZAFX_RAGGED_F64_NATIVE (measurements only, include/zafx.h).
inline RaggedAnswer ragged_route(const RouteCall& c, const RaggedBatch& b, int pcm, bool mdct_native, bool f64_native) {
    const bool lines = c.out % 128 == 0 && ft(c) && b.whole_lines;
    // k_mdct_ft32: every clip through a buffer descriptor of its own with 32-bit byte offsets (clips below 2^28 samples, d_in on 4 bytes);
    // 16-byte loads when the array is on 16 bytes and every offset and length is a multiple of 4 samples, 4-byte loads for any other
    // batch.  int16 (W = 2048 only): the 16-byte-piece form alone, and no switch of its own (ZAFX_RAGGED_PCM_NATIVE is the caller's).
    if (lines && mdct_ragged_native(c)) {
        const bool aligned = c.in % 16 == 0 && b.quads, short_enough = c.in % 4 == 0 && b.below_2_28;
        const bool route = pcm != 0 ? aligned && c.log2nf == 9 : mdct_native;
        if (b.tiles32 < (1LL << 31) && short_enough && route) return {RaggedRoute::MdctNative, aligned, kMdctRaggedTile};
    }
    // the tiled float64 kernels of W = 2048: d_in on 16 bytes, offsets and lengths free; the STFT's tiles are 8 frames
    if (pcm == 0 && c.precision == ZAFX_PRECISION_F64 && c.f64_tiled && lines && c.in % 16 == 0 && f64_native) {
        const bool stft = c.kind == ZAFX_STFT;
        if ((stft ? b.tiles8 : b.tiles16) < (1LL << 31)) return {RaggedRoute::F64Native, false, stft ? kStft64RaggedTile : kMd64RaggedTile};
    }
    if (pcm != 0 && c.kind == ZAFX_MDCT) return {RaggedRoute::PcmNotTaken};
    // k_stft_ft16 / k_mel2: k_mel2's aligned form addresses a clip with 32-bit byte offsets (clips below 2^29 samples)
    const bool on_mel2 = mel_ragged_native(c);
    const bool native = c.precision == ZAFX_PRECISION_F32 && ft(c) && c.window && lines &&
                        (c.kind == ZAFX_STFT ? stft_ragged_native(c) && (!on_mel2 || b.below_2_29) : on_mel2 && b.below_2_29);
    // (int16: the fast paths of k_mel2 and k_stft_ft16 test s0 + W <= n per frame / last <= n per tile, so every multi-sample load lies
    // inside the clip whatever its length's parity, and the tail goes sample by sample: the offsets alone must be even.  The float
    // route keeps the condition on the lengths it was measured with.)
    const bool even = c.H % 2 == 0 && c.in % 8 == 0 && b.offsets_even && (pcm != 0 || b.lengths_even);
    // (int16: W = 2048 -- k_mel2's geometry, the complex kinds of k_stft_ft16 --, even hop and offsets, d_in on 8 bytes, clips below 2^29 frames)
    if (pcm != 0 && !(native && c.log2nf == 10 && even && b.below_2_29)) return {RaggedRoute::PcmNotTaken};
    if (native) return {c.kind == ZAFX_STFT ? RaggedRoute::StftNative : RaggedRoute::MelNative, even, kStftRaggedTile};
    return {RaggedRoute::PerClip};
}

// The inverse entry points: the batch is native when the plan has the form, the array is on 4 bytes and every block passes the kind's
// test (RouteCall: T = the block's frames, as an int -- a count beyond it fails either test as INT_MAX does).
inline bool ragged_blocks_base_ok(const RouteCall& c) { return c.in % 4 == 0; }
// k_imdct: 16-byte gathers (a pitch that is a multiple of 4 floats), a block below 2^32 bytes behind its buffer descriptor
inline bool imdct_ragged_block(const RouteCall& c) { return row_pitch(c) % 4 == 0 && (long long)(c.W / 2) * row_pitch(c) * 4 < (1LL << 32); }
// k_istft_ft16: a block counted as W rows behind signed 32-bit byte offsets (istft_route's bound), frames below 2^28
inline bool istft_ragged_block(const RouteCall& c) { return c.T < (1LL << 28) && spectrum_addressable(c, c.W); }

}  // namespace zafx
