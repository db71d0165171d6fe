// What zafx_execute_masked_pcm and zafx_execute_masked_pcm_ragged refuse, asked of the entry points' own predicates (zafx_routes.hpp) without a
// device, in the entry points' order: maskfilter_pcm_call_refusal (channels, output type, the arrays' grids), then the refusals of the form
// record of the channel count -- the float stereo kind's own record for two channels.
// Build: g++ -O2 -std=c++17 -I zaf-python_amd/csrc tests/host_emu/maskfilter_pcm_routes_emu.cpp -o maskfilter_pcm_routes_emu
// stdin: lines "e kind layout n_channels mask_channels out_bytes in mask out n" (the equal-length call; in / mask / out: addresses) or
//        "r kind layout n_channels mask_channels out_bytes in mask out n_clips length_0 .. length_{n_clips-1}" (the ragged one)
// stdout: first "MASKFILTER MASKFILTER_REST bound(mono) bound(stereo, 1) bound(stereo, 2)" and the four kernel names on one line; then per line
//         "taken" or "refused <clip>: <message>" (<clip> = -1 for the equal-length call and for a refusal that is none of a clip's)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "zafx_routes.hpp"

static_assert(&zafx::maskfilter_pcm_form(2) == &zafx::kMaskfilterStereo, "two channels: the float stereo kind's record");
static_assert(zafx::kMaskfilterPcmMono.max_units == zafx::kMaskfilterReal.max_units && zafx::kMaskfilterPcmMono.too_long[0] == zafx::kMaskfilterReal.too_long[0],
              "one channel: the real kind's bound in the real kind's words");
// the samples of the longest clip taken lie behind one descriptor: 2 N bytes mono, 4 N stereo
static_assert((zafx::kMaskfilterPcmMono.max_units - 1) * 2 + 2 <= (1LL << 31) && (zafx::kMaskfilterStereo.max_units - 1) * 4 + 4 <= (1LL << 31), "");

int main() {
    std::printf("%d %d %lld %lld %lld\n", ZAFX_MASKFILTER, ZAFX_MASKFILTER_REST, (long long)zafx::maskfilter_pcm_form(1).bound(0),
                (long long)zafx::maskfilter_pcm_form(2).bound(1), (long long)zafx::maskfilter_pcm_form(2).bound(2));
    std::printf("%s %s %s %s\n", zafx::kMaskfilterPcmKernel, zafx::kMaskfilterPcmRaggedKernel, zafx::kMaskfilterStereoPcmKernel, zafx::kMaskfilterStereoPcmRaggedKernel);
    char form;
    while (std::scanf(" %c", &form) == 1) {
        int kind, layout;
        long long ch, mc, ob, in, mask, out;
        if (std::scanf("%d %d %lld %lld %lld %lld %lld %lld", &kind, &layout, &ch, &mc, &ob, &in, &mask, &out) != 8) return 2;
        std::vector<int64_t> lengths;
        long long n = 0;
        if (form == 'e') {
            if (std::scanf("%lld", &n) != 1) return 2;
        } else {
            long long n_clips;
            if (std::scanf("%lld", &n_clips) != 1 || n_clips < 0) return 2;
            lengths.resize((size_t)n_clips);
            for (auto& v : lengths) {
                long long t;
                if (std::scanf("%lld", &t) != 1) return 2;
                v = t;
            }
        }
        int64_t clip = -1;
        const char* why = zafx::maskfilter_pcm_call_refusal(ch, mc, ob, (uintptr_t)in, (uintptr_t)mask, (uintptr_t)out);
        if (!why) {
            const zafx::MaskfilterForm& f = zafx::maskfilter_pcm_form((int)ch);
            const int64_t count = ch == 2 ? mc : 0;
            if (form == 'e') {
                zafx::RouteCall c;
                c.kind = kind, c.layout = layout, c.n = n;
                why = zafx::maskfilter_form_refusal(f, c, count);
            } else {
                why = zafx::maskfilter_form_ragged_refusal(f, kind, layout, count, lengths.data(), (int64_t)lengths.size(), &clip);
            }
        }
        if (why) std::printf("refused %lld: %s\n", (long long)clip, why);
        else std::printf("taken\n");
    }
    return 0;
}
