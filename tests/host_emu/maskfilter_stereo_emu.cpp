// CPU emulation of k_maskfilter_stereo (zafx_maskfilter_stereo.hip): the packed stereo transform z = L + i R, the caller's mask(s) on the pairs
// (k, W-k) -- maskfilter_stereo_pair (a mask per channel) or maskfilter_stereo_pair_shared (one mask), zafx_maskfilter_stereo.hpp --, the
// inverse transform on the forward core and the two-term overlap-add -- "threads" are loops, arithmetic in float32 as on the device.
// Build: g++ -O2 -std=c++17 -DZAFX_HOST_EMU -I zaf-python_amd/csrc tests/host_emu/maskfilter_stereo_emu.cpp -o maskfilter_stereo_emu
// stdin:  int32 W, int32 N, int32 mask_channels (1 or 2), float32 window[W], float32 x[N][2], float32 mask[mask_channels][W/2+1][T]
//         (T = ceil(N / (W/2)) + 1)
// stdout: float32 y[N][2]
#include <cstdio>
#include <vector>

#include "zafx_maskfilter_stereo.hpp"
#include "zafx_twiddle.hpp"
#include "fft_runner.hpp"

using namespace zafx;

template <int LOG2W>
static void run(const std::vector<float>& win, const std::vector<float>& x, const std::vector<float>& mask, int mc, long long n, std::vector<float>& out) {
    constexpr int LOG2E = maskfilter_stereo_log2e(LOG2W);
    using C = FftCfg<LOG2W, LOG2E>;
    constexpr int W = C::N, H = W / 2;
    const auto twv = build_pass_twiddles(LOG2W, LOG2E);
    std::vector<float2> tw(twv.size() + 1);
    for (size_t i = 0; i < twv.size(); ++i) tw[i] = make_float2(twv[i].re, twv[i].im);
    double g = 0;
    for (int i = 0; i < W; i += H) g += (double)win[(size_t)i];
    const float gain = 1.f / ((float)W * (float)g);
    const long long blocks = (n + H - 1) / H, T = maskfilter_frames(n, W);
    auto m = [&](int c, int k, long long t) { return mask[((size_t)c * (H + 1) + (size_t)k) * (size_t)T + (size_t)t]; };
    std::vector<float2> regs((size_t)W), buf((size_t)C::PITCH), prev((size_t)H);
    for (long long j = 0; j <= blocks; ++j) {   // frame j: sample frames (j - 1) H .. (j + 1) H - 1
        for (int p = 0; p < C::P; ++p)
            for (int i = 0; i < C::E; ++i) {
                const int k = p + i * C::P;
                const long long s = (j - 1) * H + k;
                const float2 z = s >= 0 && s < n ? make_float2(x[(size_t)(2 * s)], x[(size_t)(2 * s + 1)]) : make_float2(0.f, 0.f);
                regs[(size_t)p * C::E + i] = cscale(z, win[(size_t)k]);
            }
        Runner<LOG2W, LOG2E, 0>::run(regs, buf, tw.data());
        for (int k = 0; k <= H; ++k) {
            const int pk = phys_t<C::PS>(k), pn = phys_t<C::PS>((W - k) & (W - 1));
            float2 ck, cn;
            if (mc == 2) maskfilter_stereo_pair(buf[(size_t)pk], buf[(size_t)pn], m(0, k, j), m(1, k, j), ck, cn);
            else maskfilter_stereo_pair_shared(buf[(size_t)pk], buf[(size_t)pn], m(0, k, j), ck, cn);
            buf[(size_t)pk] = center_swap(ck);
            buf[(size_t)pn] = center_swap(cn);
        }
        for (int p = 0; p < C::P; ++p) regs_read<LOG2W, LOG2E>(&regs[(size_t)p * C::E], buf.data(), p);
        Runner<LOG2W, LOG2E, 0>::run(regs, buf, tw.data());
        if (j > 0)
            for (int k = 0; k < H; ++k) {
                const long long s = (j - 1) * H + k;
                if (s >= n) break;
                const float2 y = center_swap(cscale(cadd(prev[(size_t)k], buf[(size_t)phys_t<C::PS>(k)]), gain));
                out[(size_t)(2 * s)] = y.x;
                out[(size_t)(2 * s + 1)] = y.y;
            }
        for (int k = 0; k < H; ++k) prev[(size_t)k] = buf[(size_t)phys_t<C::PS>(H + k)];
    }
}

int main() {
    int hdr[3];
    if (fread(hdr, sizeof(int), 3, stdin) != 3) return 2;
    const int w = hdr[0], mc = hdr[2];
    const long long n = hdr[1];
    if (w < 2 || n < 0 || (mc != 1 && mc != 2)) return 3;
    const long long frames = maskfilter_frames(n, w);
    std::vector<float> win((size_t)w), x((size_t)(2 * n)), out((size_t)(2 * n), 0.f);
    std::vector<float> mask((size_t)mc * (size_t)(w / 2 + 1) * (size_t)frames);
    if (fread(win.data(), sizeof(float), win.size(), stdin) != win.size()) return 2;
    if (x.size() && fread(x.data(), sizeof(float), x.size(), stdin) != x.size()) return 2;
    if (fread(mask.data(), sizeof(float), mask.size(), stdin) != mask.size()) return 2;
    switch (w) {
        case 256: run<8>(win, x, mask, mc, n, out); break;
        case 512: run<9>(win, x, mask, mc, n, out); break;
        case 1024: run<10>(win, x, mask, mc, n, out); break;
        case 2048: run<11>(win, x, mask, mc, n, out); break;
        default: return 3;
    }
    return fwrite(out.data(), sizeof(float), out.size(), stdout) == out.size() ? 0 : 4;
}
