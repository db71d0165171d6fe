// mdct_fold_emu.cpp -- the forward MDCT's sign-folded window table (zafx_wfold.hpp, what finalize_constant uploads as d_wfold) and the fold,
// pack and tap pairing of k_mdct_ft32, restated in double and held to the direct definition of the MDCT on ANY window:
//     table  (w0, w1, w2, w3)[m] = mdct_fold_window(w)            -- the library's own function, its float32 values taken as they are
//     fold   re = x[a] w0 + x[b] w1,  im = x[c] w2 + x[d] w3      -- taps (a, b, c, d) of packed input m, both branches of 2m < nf
//     pack   c[m] = (re + i im) g_m,  g_m = exp(-i pi (8m+1) / (8M)),  M = W/2
//     FFT    Y = DFT_{M/2}(c)                                      -- a naive O(n^2) DFT
//     post   y_k = Y[k] g_k ;  X[2k] = Re y_k ;  X[M-1-2k] = -Im y_k
// against  X[k] = sum_n x[n] w[n] cos(2 pi / W (n + 1/2 + W/4)(k + 1/2)).  Under KBD or the sine window the table's components are pairwise
// equal in magnitude (mirror taps), so a swapped pair or a tap at its mirror position passes every test on those windows; here it does not.
//
// stdin: int32 W, then W float32 window taps.  stdout: "W max|X - direct| / max|direct|".  Exit status 1 above 1e-11.
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "zafx_wfold.hpp"

using cd = std::complex<double>;

static double unit(uint64_t& s) {   // a fixed sequence in (-1, 1)
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(int64_t)(s >> 11) / (double)(1ll << 52) - 1.0;
}

int main() {
    int32_t W = 0;
    if (std::fread(&W, sizeof W, 1, stdin) != 1 || W < 8 || W % 8) return 2;
    std::vector<float> w((size_t)W);
    if (std::fread(w.data(), sizeof(float), (size_t)W, stdin) != (size_t)W) return 2;
    const int nf = W / 4, M = W / 2;
    const double pi = std::acos(-1.0);
    std::vector<double> x((size_t)W);
    uint64_t seed = 0x5eed0000u + (uint64_t)W;
    for (double& v : x) v = unit(seed);

    const std::vector<float> wf = zafx::mdct_fold_window(w.data(), W);
    std::vector<cd> c((size_t)nf), Y((size_t)nf);
    for (int m = 0; m < nf; ++m) {
        const zafx::MdctFoldTaps t = zafx::mdct_fold_taps(nf, m);
        const float* q = &wf[(size_t)m * 4];
        const double re = x[t.a] * (double)q[0] + x[t.b] * (double)q[1], im = x[t.c] * (double)q[2] + x[t.d] * (double)q[3];
        c[m] = cd(re, im) * std::polar(1.0, -pi * (8.0 * m + 1.0) / (8.0 * M));
    }
    for (int k = 0; k < nf; ++k) {
        cd s = 0;
        for (int m = 0; m < nf; ++m) s += c[m] * std::polar(1.0, -2.0 * pi * (double)((long long)k * m % nf) / nf);
        Y[k] = s;
    }
    std::vector<double> X((size_t)M);
    for (int k = 0; k < nf; ++k) {
        const cd y = Y[k] * std::polar(1.0, -pi * (8.0 * k + 1.0) / (8.0 * M));
        X[2 * k] = y.real();
        X[M - 1 - 2 * k] = -y.imag();
    }
    double err = 0, peak = 0;
    for (int k = 0; k < M; ++k) {
        double d = 0;
        for (int n = 0; n < W; ++n) d += x[n] * (double)w[n] * std::cos(2.0 * pi / W * (n + 0.5 + W / 4.0) * (k + 0.5));
        err = std::fmax(err, std::fabs(X[k] - d));
        peak = std::fmax(peak, std::fabs(d));
    }
    const double rel = peak > 0 ? err / peak : err;
    std::printf("%d %.3e\n", (int)W, rel);
    return rel <= 1e-11 ? 0 : 1;
}
