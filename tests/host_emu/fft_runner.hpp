// fft_frame<LOG2N, LOG2E> (zafx_fft.hpp) with the frame's threads as a loop: Runner<LOG2N, LOG2E, 0>::run(regs, buf, tw) transforms the frame
// whose thread p holds its E points in regs[p * E ..], through the LDS frame buf and the pass tables tw.  Shared by the emulation programs of
// this directory; needs -DZAFX_HOST_EMU and the library's source directory on the include path, as they do.
#pragma once
#include <vector>

#include "zafx_fft.hpp"

template <int LOG2N, int LOG2E, int LOG2NS>
struct Runner {
    static void run(std::vector<float2>& regs, std::vector<float2>& buf, const float2* tw) {
        using namespace zafx;
        using C = FftCfg<LOG2N, LOG2E>;
        if constexpr (LOG2NS < LOG2N) {
            constexpr int LR = pass_log2r(LOG2N - LOG2NS, LOG2E);
            for (int p = 0; p < C::P; ++p)
                pass_write<LOG2N, LOG2E, LOG2NS, LR>(&regs[(size_t)p * C::E], buf.data(), p, tw + twiddle_offset(LOG2N, LOG2E, LOG2NS));
            if constexpr (LOG2NS + LR < LOG2N) {
                for (int p = 0; p < C::P; ++p) regs_read<LOG2N, LOG2E>(&regs[(size_t)p * C::E], buf.data(), p);
                Runner<LOG2N, LOG2E, LOG2NS + LR>::run(regs, buf, tw);
            }
        }
    }
};
