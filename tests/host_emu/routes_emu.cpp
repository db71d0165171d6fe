// routes_emu: zafx_routes.hpp on the host (g++ -std=c++17, no HIP) -- what tests/test_routes_host.py and tests/test_gpu_routes.py ask.
// Reads calls from stdin, one per line, as `key=value` fields (tests/route_cases.py call_line):
//   kind f64 bluestein log2nf log2e layout spectrum W H row_align n_filters tables window16 claim mel2 n_clips n T out_len x out channels sample_bytes
// (`tables`: 1 = every twiddle / filterbank table the plan of such a geometry builds is present; a later `tw_r32` overrides that one) and prints, per line,
//   route=<name> kernel=<name | refused> aligned= vec= claimed= carry= pcm= pcm_direct= band_usable=
// pcm_direct: the family's *_pcm_direct_ok for a call with channels > 0; band_usable: mel_band_usable (the fused-mel predicate).
//
// The ragged form (tests/ragged_route_cases.py call_line) -- a line with an `entry` field: the plan fields as above (x / out: d_in / d_out), plus
//   entry (0 zafx_execute_ragged[_pcm], 1 zafx_execute_imdct_ragged, 2 zafx_execute_istft_ragged)  f64_tiled  env_pcm env_mdct env_f64 env_inverse
//   offsets= lengths= frames=   (comma-separated, one entry per clip; the inverses read `frames` alone)
// and prints
//   route=<ragged route | native | per-clip> kernel=<name | per-clip | none> aligned= tile=
// (kernel: `per-clip` runs the equal-length routes clip by clip, `none` leaves an integer batch to the convert-first path).
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "zafx_routes.hpp"

using namespace zafx;

static std::vector<long long> list_of(const char* s) {
    std::vector<long long> v;
    while (*s) {
        char* end = nullptr;
        v.push_back(std::strtoll(s, &end, 10));
        s = *end == ',' ? end + 1 : end;
    }
    return v;
}

// The kernel a native answer launches (StftNative: launch_stft_ragged hands spec2_ragged plans to k_mel2); null: no RAGGED form runs
static const char* ragged_kernel_name(const RouteCall& c, RaggedRoute r) {
    switch (r) {
        case RaggedRoute::MdctNative: return kernel_name(RaggedKernel::Mdct);
        case RaggedRoute::F64Native: return kernel_name(c.kind == ZAFX_STFT ? RaggedKernel::Stft64 : c.kind == ZAFX_MDCT ? RaggedKernel::Mdct64 : RaggedKernel::Mel64);
        case RaggedRoute::StftNative: return kernel_name(spec2_ragged(c) ? RaggedKernel::Mel2 : RaggedKernel::Stft);
        case RaggedRoute::MelNative: return kernel_name(RaggedKernel::Mel2);
        default: return nullptr;
    }
}

static const char* route_name(RaggedRoute r) {
    static const char* const names[] = {"mdct-native", "f64-native", "stft-native", "mel-native", "per-clip", "pcm-not-taken"};
    return names[(int)r];
}

// One line of the ragged form: the batch summary as zafx_capi.cpp fills it, then the header's answer.
static int ragged(RouteCall c, int entry, const std::vector<long long>& offsets, const std::vector<long long>& lengths, const std::vector<long long>& frames,
                  bool env_pcm, bool env_mdct, bool env_f64, bool env_inverse) {
    if (entry != 0) {
        bool native = (entry == 1 ? imdct_ragged_native(c) : istft_ragged_native(c)) && ragged_blocks_base_ok(c) && env_inverse;
        for (size_t i = 0; native && i < frames.size(); ++i) {
            c.T = (int)std::min<long long>(frames[i], INT32_MAX);
            native = entry == 1 ? imdct_ragged_block(c) : istft_ragged_block(c);
        }
        std::printf("route=%s kernel=%s aligned=0 tile=%d\n", native ? "native" : "per-clip",
                    native ? kernel_name(entry == 1 ? RaggedKernel::Imdct : RaggedKernel::Istft) : "per-clip", entry == 1 ? kImdctRaggedTile : kIstftRaggedTile);
        return 0;
    }
    if (offsets.size() != lengths.size() || frames.size() != lengths.size()) {
        std::fprintf(stderr, "routes_emu: offsets, lengths and frames differ in length\n");
        return 2;
    }
    const bool integers = c.channels > 0;
    const int pcm = ragged_pcm_mode(c.channels, c.sample_bytes, env_pcm);
    const int64_t elem_bytes = out_elem_bytes(c.kind, c.precision, c.spectrum);
    RaggedBatch b;
    for (size_t i = 0; i < lengths.size(); ++i) {
        b.add(offsets[i], lengths[i], frames[i], row_pitch(c.layout, c.row_align, frames[i]), elem_bytes);
        if (b.too_large()) {
            std::printf("route=too-large kernel=refused aligned=0 tile=0\n");
            return 0;
        }
    }
    RaggedAnswer a{RaggedRoute::PcmNotTaken};
    if (!integers || pcm != 0) a = ragged_route(c, b, pcm, env_mdct, env_f64);
    const char* name = ragged_kernel_name(c, a.k);
    std::printf("route=%s kernel=%s aligned=%d tile=%d\n", route_name(a.k), name ? name : a.k == RaggedRoute::PerClip ? "per-clip" : "none", (int)a.aligned, a.tile_frames);
    return 0;
}

template <class K>
static void print(const Route<K>& r, bool refused, bool pcm_direct, bool band_usable) {
    std::printf("route=%s kernel=%s aligned=%d vec=%d claimed=%d carry=%d pcm=%d pcm_direct=%d band_usable=%d\n", route_name(r.k),
                refused ? "refused" : kernel_name(r.k), (int)r.aligned, (int)r.vec, (int)r.claimed, (int)r.carry, (int)r.pcm, (int)pcm_direct, (int)band_usable);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        RouteCall c;
        int entry = -1;
        bool env_pcm = true, env_mdct = true, env_f64 = true, env_inverse = true;
        std::vector<long long> offsets, lengths, frames;
        std::istringstream in(line);
        std::string field;
        while (in >> field) {
            const size_t eq = field.find('=');
            if (eq == std::string::npos) {
                std::fprintf(stderr, "routes_emu: field without '=': %s\n", field.c_str());
                return 2;
            }
            const std::string key = field.substr(0, eq);
            const long long v = std::strtoll(field.c_str() + eq + 1, nullptr, 10);
            if (key == "kind") c.kind = (int)v;
            else if (key == "f64") c.precision = v ? ZAFX_PRECISION_F64 : ZAFX_PRECISION_F32;
            else if (key == "bluestein") c.bluestein = v != 0;
            else if (key == "log2nf") c.log2nf = (int)v;
            else if (key == "log2e") c.log2e = (int)v;
            else if (key == "layout") c.layout = (int)v;
            else if (key == "spectrum") c.spectrum = (int)v;
            else if (key == "W") c.W = (int)v;
            else if (key == "H") c.H = (int)v;
            else if (key == "row_align") c.row_align = (int)v;
            else if (key == "n_filters") c.n_filters = (int)v;
            else if (key == "tables") c.tw_pass = c.tw_aux = c.tw_r32 = c.tw_sub = c.tw_quad = c.tw_band = c.fbw = c.window = c.wfold = v != 0;
            else if (key == "tw_r32") c.tw_r32 = v != 0;
            else if (key == "window16") c.window16 = v != 0;
            else if (key == "claim") c.claim = v != 0;
            else if (key == "mel2") c.mel2 = v != 0;
            else if (key == "n_clips") c.n_clips = v;
            else if (key == "n") c.n = v;
            else if (key == "T") c.T = (int)v;
            else if (key == "out_len") c.out_len = v;
            else if (key == "x") c.in = (uintptr_t)v;
            else if (key == "out") c.out = (uintptr_t)v;
            else if (key == "channels") c.channels = (int)v;
            else if (key == "sample_bytes") c.sample_bytes = (int)v;
            else if (key == "entry") entry = (int)v;
            else if (key == "f64_tiled") c.f64_tiled = v != 0;
            else if (key == "env_pcm") env_pcm = v != 0;
            else if (key == "env_mdct") env_mdct = v != 0;
            else if (key == "env_f64") env_f64 = v != 0;
            else if (key == "env_inverse") env_inverse = v != 0;
            else if (key == "offsets") offsets = list_of(field.c_str() + eq + 1);
            else if (key == "lengths") lengths = list_of(field.c_str() + eq + 1);
            else if (key == "frames") frames = list_of(field.c_str() + eq + 1);
            else {
                std::fprintf(stderr, "routes_emu: unknown field %s\n", key.c_str());
                return 2;
            }
        }
        if (entry >= 0) {
            if (int rc = ragged(c, entry, offsets, lengths, frames, env_pcm, env_mdct, env_f64, env_inverse)) return rc;
            continue;
        }
        switch (c.kind) {
            case ZAFX_STFT: print(stft_route(c), false, stft_pcm_direct_ok(c) || pcm_direct_ok(c), false); break;
            case ZAFX_ISTFT: print(istft_route(c), false, false, false); break;
            case ZAFX_MDCT: print(mdct_route(c), false, mdct_pcm_direct_ok(c), false); break;
            case ZAFX_IMDCT: print(imdct_route(c), false, false, false); break;
            case ZAFX_MEL:
            case ZAFX_MFCC: print(mel_route(c), false, pcm_direct_ok(c), mel_band_usable(c)); break;
            case ZAFX_CQT:
            case ZAFX_CHROMA:
                std::printf("route=cqt kernel=%s aligned=0 vec=0 claimed=0 carry=0 pcm=0 pcm_direct=0 band_usable=0\n", cqt_clip_refused(c) ? "refused" : kCqtKernel);
                break;
            case ZAFX_CENTER:
            case ZAFX_CENTER_SIDES:
                std::printf("route=center kernel=%s aligned=0 vec=0 claimed=0 carry=0 pcm=0 pcm_direct=0 band_usable=0\n", center_clip_refused(c) ? "refused" : kCenterKernel);
                break;
            default: std::fprintf(stderr, "routes_emu: unknown kind %d\n", c.kind); return 2;
        }
    }
    return 0;
}
