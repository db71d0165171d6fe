// zafx_wfold.hpp -- the sign-folded window table of the forward MDCT kernels (k_mdct_ft32 and its b / bc / q / ragged / PCM forms), host side.
// Plain C++: finalize_constant (zafx_capi.cpp) packs the plan's d_wfold with it, and tests/host_emu/mdct_fold_emu.cpp compiles it with g++ to
// check the table, the fold and the tap pairing against the direct MDCT on windows that are not mirror-symmetric.
#pragma once

#include <cstddef>
#include <vector>

namespace zafx {

// The samples that packed input m of a frame of W = 4 nf samples reads (fold + pack of zafx_mdct.hip: v = (-c_r - d, a - b_r),
// c[m] = v[2m] + i v[M-1-2m]): re = x[a] w0 + x[b] w1, im = x[c] w2 + x[d] w3 with (w0, w1, w2, w3) quadruple m of the table below.
struct MdctFoldTaps { int a, b, c, d; };
inline MdctFoldTaps mdct_fold_taps(int nf, int m) {
    if (2 * m < nf) return {3 * nf - 1 - 2 * m, 3 * nf + 2 * m, nf - 1 - 2 * m, nf + 2 * m};
    return {2 * m - nf, 3 * nf - 1 - 2 * m, nf + 2 * m, 5 * nf - 1 - 2 * m};
}

// Sign-folded window for the fold + pack step of k_mdct_ft32: quadruple m holds the window at the four taps of mdct_fold_taps(nf, m), each
// with the sign the fold gives its sample.  w: W = 4 nf taps; -> nf quadruples.  Components 0 / 3 and 1 / 2 (either branch) sit at mirror
// positions n and W-1-n of the window: equal in magnitude under KBD or the sine window, and under no window that is not symmetric.
inline std::vector<float> mdct_fold_window(const float* w, int window_length) {
    const int nf = window_length / 4;
    std::vector<float> wf((size_t)nf * 4);
    for (int m = 0; m < nf; ++m) {
        float* o = &wf[(size_t)m * 4];
        if (2 * m < nf) {
            o[0] = -w[3 * nf - 1 - 2 * m]; o[1] = -w[3 * nf + 2 * m];
            o[2] = w[nf - 1 - 2 * m];      o[3] = -w[nf + 2 * m];
        } else {
            o[0] = w[2 * m - nf];          o[1] = -w[3 * nf - 1 - 2 * m];
            o[2] = -w[nf + 2 * m];         o[3] = -w[5 * nf - 1 - 2 * m];
        }
    }
    return wf;
}

}  // namespace zafx
