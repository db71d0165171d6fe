// What zafx_execute_masked_stems_ragged refuses, asked of the entry point's own predicate (maskfilter_stems_ragged_refusal, zafx_routes.hpp)
// without a device.
// Build: g++ -O2 -std=c++17 -I zaf-python_amd/csrc tests/host_emu/maskfilter_stems_ragged_routes_emu.cpp -o maskfilter_stems_ragged_routes_emu
// stdin: lines "kind layout n_stems n_clips length_0 .. length_{n_clips-1}"     stdout: per line "taken" or "refused <clip>: <message>"
#include <cstdint>
#include <cstdio>
#include <vector>

#include "zafx_routes.hpp"

int main() {
    std::printf("%d %d %d\n", ZAFX_MASKFILTER, ZAFX_MASKFILTER_REST, zafx::kMaskfilterMaxStems);
    int kind, layout;
    long long stems, n_clips;
    while (std::scanf("%d %d %lld %lld", &kind, &layout, &stems, &n_clips) == 4) {
        std::vector<int64_t> lengths((size_t)n_clips);
        for (auto& v : lengths) {
            long long t;
            if (std::scanf("%lld", &t) != 1) return 2;
            v = t;
        }
        int64_t clip = -2;
        const char* why = zafx::maskfilter_stems_ragged_refusal(kind, layout, stems, lengths.data(), n_clips, &clip);
        if (why) std::printf("refused %lld: %s\n", (long long)clip, why);
        else std::printf("taken\n");
    }
    return 0;
}
