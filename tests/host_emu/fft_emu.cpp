// CPU emulation of the LDS Stockham FFT core (zafx_fft.hpp) -- "threads" are loops.
// Build: g++ -O2 -std=c++17 -DZAFX_HOST_EMU -I zaf-python_amd/csrc tests/host_emu/fft_emu.cpp -o fft_emu
// Prints max normwise error vs a float64 naive DFT for every (log2n, log2e) the kernels use.
// fft_emu LOG2N LOG2E IN OUT: transforms the frames of IN (complex64, N points each, back to back) with that core and writes them to OUT
// (tests/test_accuracy_host.py holds them to a plain single-precision transform of the same frames).
// fft_emu chain LOG2N LOG2E IN OUT: the same with the chained-twiddle passes k_cqt runs (pass_write_chain: two-level root table + product tree).
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "zafx_twiddle.hpp"
#include "fft_runner.hpp"

using namespace zafx;

// The passes of fft_frame_chain (every pass pass_write_chain: no 1024-point wave-local form here).
template <int LOG2N, int LOG2E, int LOG2NS>
struct ChainRunner {
    static void run(std::vector<float2>& regs, std::vector<float2>& buf, const TwoLevelTw& t) {
        using C = FftCfg<LOG2N, LOG2E>;
        if constexpr (LOG2NS < LOG2N) {
            constexpr int LR = pass_log2r(LOG2N - LOG2NS, LOG2E);
            for (int p = 0; p < C::P; ++p) pass_write_chain<LOG2N, LOG2E, LOG2NS, LR>(&regs[(size_t)p * C::E], buf.data(), p, t);
            if constexpr (LOG2NS + LR < LOG2N) {
                for (int p = 0; p < C::P; ++p) regs_read<LOG2N, LOG2E>(&regs[(size_t)p * C::E], buf.data(), p);
                ChainRunner<LOG2N, LOG2E, LOG2NS + LR>::run(regs, buf, t);
            }
        }
    }
};

// One frame through the core: x[n] in natural order -> X[k] in natural order.  CHAIN: tw is the two-level root table.
template <int LOG2N, int LOG2E, bool CHAIN = false>
void transform(const float2* x, float2* out, const float2* tw) {
    using C = FftCfg<LOG2N, LOG2E>;
    std::vector<float2> regs((size_t)C::N), buf((size_t)C::PITCH);
    for (int p = 0; p < C::P; ++p)
        for (int i = 0; i < C::E; ++i) regs[(size_t)p * C::E + i] = x[p + i * C::P];
    if constexpr (CHAIN) ChainRunner<LOG2N, LOG2E, 0>::run(regs, buf, TwoLevelTw{tw, tw + two_level_hi_count(LOG2N)});
    else Runner<LOG2N, LOG2E, 0>::run(regs, buf, tw);
    for (int k = 0; k < C::N; ++k) out[k] = buf[phys_t<C::PS>(k)];
}

template <int LOG2N, int LOG2E, bool CHAIN = false>
int file_mode(const char* in_path, const char* out_path) {
    using C = FftCfg<LOG2N, LOG2E>;
    auto twv = CHAIN ? build_two_level_twiddles(LOG2N) : build_pass_twiddles(LOG2N, LOG2E);
    std::vector<float2> tw(twv.size() + 1);
    for (size_t i = 0; i < twv.size(); ++i) tw[i] = make_float2(twv[i].re, twv[i].im);
    FILE* in = fopen(in_path, "rb");
    FILE* out = fopen(out_path, "wb");
    if (!in || !out) return 2;
    std::vector<float2> x((size_t)C::N), y((size_t)C::N);
    size_t frames = 0;
    while (fread(x.data(), sizeof(float2), (size_t)C::N, in) == (size_t)C::N) {
        transform<LOG2N, LOG2E, CHAIN>(x.data(), y.data(), tw.data());
        if (fwrite(y.data(), sizeof(float2), (size_t)C::N, out) != (size_t)C::N) return 2;
        ++frames;
    }
    fclose(in);
    if (fclose(out)) return 2;
    printf("log2n=%d log2e=%d frames=%zu\n", LOG2N, LOG2E, frames);
    return frames ? 0 : 2;
}

#define ZAFX_EMU_SIZES(X) X(4, 1) X(5, 1) X(6, 1) X(7, 1) X(8, 2) X(9, 3) X(10, 4) X(10, 5) X(9, 5) X(11, 4) X(12, 4) X(14, 4)
// k_cqt's fully chained transforms: N = fft_length / 2 complex points for fft_length 512 ... 16384 but 2048 (its N = 1024 runs the wave-local form; 32768 and 65536 chain their first pass only)
#define ZAFX_EMU_CHAIN_SIZES(X) X(8, 2) X(9, 3) X(11, 4) X(12, 4) X(13, 4)

template <int LOG2N, int LOG2E>
double check() {
    using C = FftCfg<LOG2N, LOG2E>;
    std::vector<std::complex<double>> x(C::N), ref(C::N);
    srand(LOG2N * 131 + LOG2E);
    for (auto& v : x) v = {rand() / (double)RAND_MAX - 0.5, rand() / (double)RAND_MAX - 0.5};
    for (int k = 0; k < C::N; ++k) {
        std::complex<double> s = 0;
        for (int n = 0; n < C::N; ++n) s += x[n] * std::polar(1.0, -2.0 * M_PI * (double)((long long)n * k % C::N) / C::N);
        ref[k] = s;
    }
    auto twv = build_pass_twiddles(LOG2N, LOG2E);
    std::vector<float2> tw(twv.size() + 1);
    for (size_t i = 0; i < twv.size(); ++i) tw[i] = make_float2(twv[i].re, twv[i].im);
    std::vector<float2> regs((size_t)C::N), buf((size_t)C::PITCH);
    for (int p = 0; p < C::P; ++p)
        for (int i = 0; i < C::E; ++i) regs[(size_t)p * C::E + i] = make_float2((float)x[p + i * C::P].real(), (float)x[p + i * C::P].imag());
    Runner<LOG2N, LOG2E, 0>::run(regs, buf, tw.data());
    double err = 0, mx = 0;
    for (int k = 0; k < C::N; ++k) {
        std::complex<double> got(buf[phys_t<C::PS>(k)].x, buf[phys_t<C::PS>(k)].y);
        err = std::max(err, std::abs(got - ref[k]));
        mx = std::max(mx, std::abs(ref[k]));
    }
    printf("log2n=%d log2e=%d P=%d tw=%d relerr=%.3e\n", LOG2N, LOG2E, C::P, C::TW, err / mx);
    return err / mx;
}

int main(int argc, char** argv) {
    if (argc == 5) {
        int n = atoi(argv[1]), e = atoi(argv[2]);
#define ZAFX_EMU_FILE(N_, E_) if (n == N_ && e == E_) return file_mode<N_, E_>(argv[3], argv[4]);
        ZAFX_EMU_SIZES(ZAFX_EMU_FILE)
        fprintf(stderr, "no such core: log2n=%d log2e=%d\n", n, e);
        return 2;
    }
    if (argc == 6 && !strcmp(argv[1], "chain")) {
        int n = atoi(argv[2]), e = atoi(argv[3]);
#define ZAFX_EMU_CHAIN(N_, E_) if (n == N_ && e == E_) return file_mode<N_, E_, true>(argv[4], argv[5]);
        ZAFX_EMU_CHAIN_SIZES(ZAFX_EMU_CHAIN)
        fprintf(stderr, "no such chained core: log2n=%d log2e=%d\n", n, e);
        return 2;
    }
    if (argc == 2 && !strcmp(argv[1], "--chain-sizes")) {
#define ZAFX_EMU_CHAIN_NAME(N_, E_) printf("%d %d\n", N_, E_);
        ZAFX_EMU_CHAIN_SIZES(ZAFX_EMU_CHAIN_NAME)
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "--sizes")) {
#define ZAFX_EMU_NAME(N_, E_) printf("%d %d\n", N_, E_);
        ZAFX_EMU_SIZES(ZAFX_EMU_NAME)
        return 0;
    }
    double worst = 0;
    worst = std::max(worst, check<4, 1>());
    worst = std::max(worst, check<5, 1>());
    worst = std::max(worst, check<6, 1>());
    worst = std::max(worst, check<7, 1>());
    worst = std::max(worst, check<8, 2>());
    worst = std::max(worst, check<9, 3>());
    worst = std::max(worst, check<10, 4>());
    worst = std::max(worst, check<10, 5>());   // two radix-32 passes
    worst = std::max(worst, check<9, 5>());    // 32 x 16
    worst = std::max(worst, check<11, 4>());
    worst = std::max(worst, check<12, 4>());
    worst = std::max(worst, check<14, 4>());
    printf("worst=%.3e\n", worst);
    return worst < 2e-6 ? 0 : 1;
}
