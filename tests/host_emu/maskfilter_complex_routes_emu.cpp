// What zafx_execute_masked_complex and zafx_execute_masked_complex_ragged refuse, asked of the entry points' own predicates
// (maskfilter_complex_refusal, maskfilter_complex_ragged_refusal, zafx_routes.hpp) without a device, and the offset arithmetic at the bound:
// the compact TF complex64 mask of the longest clip taken ends below 2^31 bytes at every window, the next power of two does not.
// Build: g++ -O2 -std=c++17 -I zaf-python_amd/csrc tests/host_emu/maskfilter_complex_routes_emu.cpp -o maskfilter_complex_routes_emu
// stdin: lines "e kind layout n" (the equal-length call) or "r kind layout n_clips length_0 .. length_{n_clips-1}" (the ragged one)
// stdout: first "MASKFILTER MASKFILTER_REST bound" and per window "W mask_bytes(bound - 1) mask_bytes(2 bound)"; then per line "taken" or
//         "refused <clip>: <message>" (<clip> = -1 for the equal-length call and for a refusal that is none of a clip's)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "zafx_maskfilter.hpp"
#include "zafx_routes.hpp"

// the kernel's descriptor ends at (n_blocks + 1)(H + 1) 8 bytes, n_blocks + 1 = maskfilter_frames: the routes header counts the same bytes
template <int W>
constexpr bool bound_holds() {
    constexpr int64_t top = zafx::kMaskfilterComplexMaxSamples - 1;
    static_assert(zafx::maskfilter_frames(top, W) * (W / 2 + 1) * 8 == zafx::maskfilter_complex_mask_bytes(top, W), "one count of the mask's bytes");
    static_assert(zafx::maskfilter_frames(top, W) * (W / 2 + 1) * 8 < (1LL << 31), "the mask of the longest clip taken stays behind signed 32-bit byte offsets");
    return true;
}
static_assert(bound_holds<256>() && bound_holds<512>() && bound_holds<1024>() && bound_holds<2048>(), "");
static_assert(zafx::kMaskfilterComplexMaxSamples == (1LL << 27), "the bound the header states");

int main() {
    std::printf("%d %d %lld\n", ZAFX_MASKFILTER, ZAFX_MASKFILTER_REST, (long long)zafx::kMaskfilterComplexMaxSamples);
    for (int w : {256, 512, 1024, 2048})
        std::printf("%d %lld %lld\n", w, (long long)zafx::maskfilter_complex_mask_bytes(zafx::kMaskfilterComplexMaxSamples - 1, w),
                    (long long)zafx::maskfilter_complex_mask_bytes(2 * zafx::kMaskfilterComplexMaxSamples, w));
    char form;
    int kind, layout;
    while (std::scanf(" %c %d %d", &form, &kind, &layout) == 3) {
        const char* why = nullptr;
        int64_t clip = -1;
        if (form == 'e') {
            long long n;
            if (std::scanf("%lld", &n) != 1) return 2;
            zafx::RouteCall c;
            c.kind = kind, c.layout = layout, c.n = n;
            why = zafx::maskfilter_complex_refusal(c);
        } else {
            long long n_clips;
            if (std::scanf("%lld", &n_clips) != 1) return 2;
            std::vector<int64_t> lengths((size_t)n_clips);
            for (auto& v : lengths) {
                long long t;
                if (std::scanf("%lld", &t) != 1) return 2;
                v = t;
            }
            clip = -2;
            why = zafx::maskfilter_complex_ragged_refusal(kind, layout, lengths.data(), n_clips, &clip);
        }
        if (why) std::printf("refused %lld: %s\n", (long long)clip, why);
        else std::printf("taken\n");
    }
    return 0;
}
