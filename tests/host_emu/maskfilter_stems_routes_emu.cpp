// What zafx_execute_masked_stems refuses, asked of the launcher's own predicate (maskfilter_stems_refusal, zafx_routes.hpp) without a device.
// Build: g++ -O2 -std=c++17 -I zaf-python_amd/csrc tests/host_emu/maskfilter_stems_routes_emu.cpp -o maskfilter_stems_routes_emu
// stdin: lines "layout n_stems n_in"        stdout: per line "taken" or "refused: <message>"; first line: the kernel's name and the stem bound
#include <cstdio>

#include "zafx_routes.hpp"

int main() {
    std::printf("%s %d\n", zafx::kMaskfilterStemsKernel, zafx::kMaskfilterMaxStems);
    int layout;
    long long stems, n;
    while (std::scanf("%d %lld %lld", &layout, &stems, &n) == 3) {
        zafx::RouteCall c;
        c.kind = ZAFX_MASKFILTER, c.layout = layout, c.n = n, c.n_clips = 1;
        const char* why = zafx::maskfilter_stems_refusal(c, stems);
        if (why) std::printf("refused: %s\n", why);
        else std::printf("taken\n");
    }
    return 0;
}
