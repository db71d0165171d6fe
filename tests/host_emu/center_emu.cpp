// CPU emulation of k_center (zafx_center.hip): the packed stereo transform, split / mask / re-pack (zafx_center.hpp), the inverse
// transform on the forward core and the two-term overlap-add -- "threads" are loops, arithmetic in float32 as on the device.
// Build: g++ -O2 -std=c++17 -DZAFX_HOST_EMU -I zaf-python_amd/csrc tests/host_emu/center_emu.cpp -o center_emu
// stdin:  int32 W, int32 N, float32 window[W], float32 x[N][2]        stdout: float32 center[N][2]
#include <cstdio>
#include <vector>

#include "zafx_center.hpp"
#include "zafx_twiddle.hpp"
#include "fft_runner.hpp"

using namespace zafx;

template <int LOG2W>
static void run(const std::vector<float>& win, const std::vector<float>& x, long long n, std::vector<float>& out) {
    constexpr int LOG2E = center_log2e(LOG2W);
    using C = FftCfg<LOG2W, LOG2E>;
    constexpr int W = C::N, H = W / 2;
    const auto twv = build_pass_twiddles(LOG2W, LOG2E);
    std::vector<float2> tw(twv.size() + 1);
    for (size_t i = 0; i < twv.size(); ++i) tw[i] = make_float2(twv[i].re, twv[i].im);
    double g = 0;
    for (int i = 0; i < W; i += H) g += (double)win[(size_t)i];
    const float gain = 1.f / ((float)W * (float)g);
    const long long blocks = (n + H - 1) / H;
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
            center_pair(buf[(size_t)pk], buf[(size_t)pn], ck, cn);
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
    int hdr[2];
    if (fread(hdr, sizeof(int), 2, stdin) != 2) return 2;
    const int w = hdr[0];
    const long long n = hdr[1];
    std::vector<float> win((size_t)w), x((size_t)(2 * n)), out((size_t)(2 * n), 0.f);
    if (fread(win.data(), sizeof(float), win.size(), stdin) != win.size()) return 2;
    if (fread(x.data(), sizeof(float), x.size(), stdin) != x.size()) return 2;
    switch (w) {
        case 256: run<8>(win, x, n, out); break;
        case 512: run<9>(win, x, n, out); break;
        case 1024: run<10>(win, x, n, out); break;
        case 2048: run<11>(win, x, n, out); break;
        default: return 3;
    }
    return fwrite(out.data(), sizeof(float), out.size(), stdout) == out.size() ? 0 : 4;
}
