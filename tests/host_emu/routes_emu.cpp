// routes_emu: zafx_routes.hpp on the host (g++ -std=c++17, no HIP) -- what tests/test_routes_host.py and tests/test_gpu_routes.py ask.
// Reads calls from stdin, one per line, as `key=value` fields (tests/route_cases.py call_line):
//   kind f64 bluestein log2nf log2e layout spectrum W H row_align n_filters tables window16 claim mel2 n_clips n T out_len x out channels sample_bytes
// (`tables`: 1 = every twiddle / filterbank table the plan of such a geometry builds is present) and prints, per line,
//   route=<name> kernel=<name | refused> aligned= vec= claimed= carry= pcm= pcm_direct= band_usable=
// pcm_direct: the family's *_pcm_direct_ok for a call with channels > 0; band_usable: mel_band_usable (the fused-mel predicate).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "zafx_routes.hpp"

using namespace zafx;

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
            else if (key == "tables") c.tw_pass = c.tw_aux = c.tw_r32 = c.tw_sub = c.tw_quad = c.tw_band = c.fbw = v != 0;
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
            else {
                std::fprintf(stderr, "routes_emu: unknown field %s\n", key.c_str());
                return 2;
            }
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
