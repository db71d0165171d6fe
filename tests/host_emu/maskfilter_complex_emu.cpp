// CPU emulation of k_maskfilter_c (zafx_maskfilter.hip): two neighbouring frames of a mono clip in one complex transform, split / COMPLEX
// mask / re-pack (maskfilter_pair_c, zafx_maskfilter.hpp), the inverse transform on the forward core and the two-term overlap-add --
// "threads" are loops, arithmetic in float32 as on the device.  As the kernel does, the imaginary parts of the mask at bins 0 and W/2 are
// dropped before the pair function sees them (assigned, not multiplied: NaN there does nothing).
// Build: g++ -O2 -std=c++17 -DZAFX_HOST_EMU -I zaf-python_amd/csrc tests/host_emu/maskfilter_complex_emu.cpp -o maskfilter_complex_emu
// stdin:  int32 W, int32 N, float32 window[W], float32 x[N], complex64 mask[W/2+1][T] (interleaved re, im; T = ceil(N / (W/2)) + 1)
// stdout: float32 y[N]
#include <cstdio>
#include <vector>

#include "zafx_maskfilter.hpp"
#include "zafx_twiddle.hpp"
#include "fft_runner.hpp"

using namespace zafx;

template <int LOG2W>
static void run(const std::vector<float>& win, const std::vector<float>& x, const std::vector<float2>& mask, long long n, std::vector<float>& out) {
    constexpr int LOG2E = maskfilter_log2e(LOG2W);
    using C = FftCfg<LOG2W, LOG2E>;
    constexpr int W = C::N, H = W / 2;
    const auto twv = build_pass_twiddles(LOG2W, LOG2E);
    std::vector<float2> tw(twv.size() + 1);
    for (size_t i = 0; i < twv.size(); ++i) tw[i] = make_float2(twv[i].re, twv[i].im);
    double g = 0;
    for (int i = 0; i < W; i += H) g += (double)win[(size_t)i];
    const float gain = 1.f / ((float)W * (float)g);
    const long long blocks = (n + H - 1) / H, T = maskfilter_frames(n, W);
    auto sample = [&](long long s) { return s >= 0 && s < n ? x[(size_t)s] : 0.f; };
    auto m = [&](int k, long long t) {   // a frame beyond the last has mask 0; bins 0 and H keep their real part only
        float2 v = t < T ? mask[(size_t)k * (size_t)T + (size_t)t] : make_float2(0.f, 0.f);
        if (k == 0 || k == H) v.y = 0.f;
        return v;
    };
    std::vector<float2> regs((size_t)W), buf((size_t)C::PITCH);
    std::vector<float> carry((size_t)H);
    for (long long q = 0; 2 * q <= blocks; ++q) {   // transform q: frame 2q (from sample (2q - 1) H) + i frame 2q + 1 (from sample 2q H)
        for (int p = 0; p < C::P; ++p)
            for (int i = 0; i < C::E; ++i) {
                const int k = p + i * C::P;
                const long long s = (2 * q - 1) * H + k;
                regs[(size_t)p * C::E + i] = make_float2(sample(s) * win[(size_t)k], sample(s + H) * win[(size_t)k]);
            }
        Runner<LOG2W, LOG2E, 0>::run(regs, buf, tw.data());
        for (int k = 0; k <= H; ++k) {
            const int pk = phys_t<C::PS>(k), pn = phys_t<C::PS>((W - k) & (W - 1));
            float2 ck, cn;
            maskfilter_pair_c(buf[(size_t)pk], buf[(size_t)pn], m(k, 2 * q), m(k, 2 * q + 1), ck, cn);
            buf[(size_t)pk] = center_swap(ck);
            buf[(size_t)pn] = center_swap(cn);
        }
        for (int p = 0; p < C::P; ++p) regs_read<LOG2W, LOG2E>(&regs[(size_t)p * C::E], buf.data(), p);
        Runner<LOG2W, LOG2E, 0>::run(regs, buf, tw.data());
        // swapped: .y = masked frame 2q, .x = masked frame 2q + 1
        if (q > 0)   // block 2q - 1
            for (int k = 0; k < H; ++k) {
                const long long s = (2 * q - 1) * H + k;
                if (s < n) out[(size_t)s] = (carry[(size_t)k] + buf[(size_t)phys_t<C::PS>(k)].y) * gain;
            }
        for (int k = 0; k < H; ++k) {   // block 2q
            const long long s = 2 * q * H + k;
            if (s < n) out[(size_t)s] = (buf[(size_t)phys_t<C::PS>(H + k)].y + buf[(size_t)phys_t<C::PS>(k)].x) * gain;
        }
        for (int k = 0; k < H; ++k) carry[(size_t)k] = buf[(size_t)phys_t<C::PS>(H + k)].x;
    }
}

int main() {
    int hdr[2];
    if (fread(hdr, sizeof(int), 2, stdin) != 2) return 2;
    const int w = hdr[0];
    const long long n = hdr[1];
    if (w < 2 || n < 0) return 3;
    const long long frames = maskfilter_frames(n, w);
    std::vector<float> win((size_t)w), x((size_t)n), out((size_t)n, 0.f);
    std::vector<float2> mask((size_t)(w / 2 + 1) * (size_t)frames);
    if (fread(win.data(), sizeof(float), win.size(), stdin) != win.size()) return 2;
    if (fread(x.data(), sizeof(float), x.size(), stdin) != x.size()) return 2;
    if (fread(mask.data(), sizeof(float2), mask.size(), stdin) != mask.size()) return 2;
    switch (w) {
        case 256: run<8>(win, x, mask, n, out); break;
        case 512: run<9>(win, x, mask, n, out); break;
        case 1024: run<10>(win, x, mask, n, out); break;
        case 2048: run<11>(win, x, mask, n, out); break;
        default: return 3;
    }
    return fwrite(out.data(), sizeof(float), out.size(), stdout) == out.size() ? 0 : 4;
}
