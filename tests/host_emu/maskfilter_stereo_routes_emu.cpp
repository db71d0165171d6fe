// What zafx_execute_masked_stereo and zafx_execute_masked_stereo_ragged refuse, asked of the entry points' own predicates
// (maskfilter_stereo_refusal, maskfilter_stereo_ragged_refusal, zafx_routes.hpp) without a device; the offset arithmetic at the bounds: the
// compact TF mask(s) of the longest clip taken end below 2^31 bytes at every window; and the cut of a ragged batch into the units
// k_maskfilter_stereo walks (maskfilter_stereo_cut_units, zafx_units.hpp).
// Build: g++ -O2 -std=c++17 -I zaf-python_amd/csrc tests/host_emu/maskfilter_stereo_routes_emu.cpp -o maskfilter_stereo_routes_emu
// stdin: lines "e kind layout mask_channels n" (the equal-length call), "r kind layout mask_channels n_clips length_0 .. length_{n_clips-1}"
//        (the ragged one) or "c W F slots per_slot n_clips length_0 .. length_{n_clips-1}" (the cut; clip i lies at in_off 1000 i + 1,
//        out_off 2000 i + 2, mask_off 3000 i + 3)
// stdout: first "MASKFILTER MASKFILTER_REST bound(1) bound(2)" and per window "W mask_bytes(bound(1) - 1, 1) mask_bytes(bound(2) - 1, 2)
//         mask_bytes(2 bound(1), 1) mask_bytes(2 bound(2), 2)"; then per e / r line "taken" or "refused <clip>: <message>" (<clip> = -1 for
//         the equal-length call and for a refusal that is none of a clip's), per c line "units <count>" followed by one line
//         "in_off n_samples out_off mask_off b0 b1 mask_pitch" per unit
#include <cstdint>
#include <cstdio>
#include <vector>

#include "zafx_maskfilter.hpp"
#include "zafx_routes.hpp"
#include "zafx_units.hpp"

// the kernel's descriptor ends at (n_blocks + 1) mask_channels (H + 1) 4 bytes, n_blocks + 1 = maskfilter_frames: the routes header counts the same bytes
template <int W, int MC>
constexpr bool bound_holds() {
    constexpr int64_t top = zafx::maskfilter_stereo_max_frames(MC) - 1;
    static_assert(zafx::maskfilter_frames(top, W) * MC * (W / 2 + 1) * 4 == zafx::maskfilter_stereo_mask_bytes(top, W, MC), "one count of the masks' bytes");
    static_assert(zafx::maskfilter_frames(top, W) * MC * (W / 2 + 1) * 4 < (1LL << 31), "the masks of the longest clip taken stay behind signed 32-bit byte offsets");
    static_assert(top * 8 + 8 <= (1LL << 31), "the samples of the longest clip taken lie behind one descriptor");
    return true;
}
static_assert(bound_holds<256, 1>() && bound_holds<512, 1>() && bound_holds<1024, 1>() && bound_holds<2048, 1>(), "");
static_assert(bound_holds<256, 2>() && bound_holds<512, 2>() && bound_holds<1024, 2>() && bound_holds<2048, 2>(), "");
static_assert(zafx::maskfilter_stereo_max_frames(1) == (1LL << 28) && zafx::maskfilter_stereo_max_frames(2) == (1LL << 27), "the bounds the header states");

static bool read_lengths(std::vector<int64_t>& lengths) {
    long long n_clips;
    if (std::scanf("%lld", &n_clips) != 1 || n_clips < 0) return false;
    lengths.resize((size_t)n_clips);
    for (auto& v : lengths) {
        long long t;
        if (std::scanf("%lld", &t) != 1) return false;
        v = t;
    }
    return true;
}

int main() {
    std::printf("%d %d %lld %lld\n", ZAFX_MASKFILTER, ZAFX_MASKFILTER_REST, (long long)zafx::maskfilter_stereo_max_frames(1), (long long)zafx::maskfilter_stereo_max_frames(2));
    for (int w : {256, 512, 1024, 2048})
        std::printf("%d %lld %lld %lld %lld\n", w, (long long)zafx::maskfilter_stereo_mask_bytes(zafx::maskfilter_stereo_max_frames(1) - 1, w, 1),
                    (long long)zafx::maskfilter_stereo_mask_bytes(zafx::maskfilter_stereo_max_frames(2) - 1, w, 2),
                    (long long)zafx::maskfilter_stereo_mask_bytes(2 * zafx::maskfilter_stereo_max_frames(1), w, 1),
                    (long long)zafx::maskfilter_stereo_mask_bytes(2 * zafx::maskfilter_stereo_max_frames(2), w, 2));
    char form;
    while (std::scanf(" %c", &form) == 1) {
        std::vector<int64_t> lengths;
        if (form == 'c') {
            int W, F, per_slot;
            long long slots;
            if (std::scanf("%d %d %lld %d", &W, &F, &slots, &per_slot) != 4 || !read_lengths(lengths)) return 2;
            std::vector<int64_t> in_off(lengths.size()), out_off(lengths.size()), mask_off(lengths.size());
            for (size_t i = 0; i < lengths.size(); ++i) in_off[i] = 1000 * (int64_t)i + 1, out_off[i] = 2000 * (int64_t)i + 2, mask_off[i] = 3000 * (int64_t)i + 3;
            const auto units = zafx::maskfilter_stereo_cut_units(lengths.data(), in_off.data(), out_off.data(), mask_off.data(), (int64_t)lengths.size(), W, F, slots, per_slot);
            std::printf("units %zu\n", units.size());
            for (const auto& u : units) std::printf("%lld %lld %lld %lld %d %d %d\n", u.in_off, u.n_samples, u.out_off, u.mask_off, u.b0, u.b1, u.mask_pitch);
            continue;
        }
        int kind, layout, mc;
        if (std::scanf("%d %d %d", &kind, &layout, &mc) != 3) return 2;
        const char* why = nullptr;
        int64_t clip = -1;
        if (form == 'e') {
            long long n;
            if (std::scanf("%lld", &n) != 1) return 2;
            zafx::RouteCall c;
            c.kind = kind, c.layout = layout, c.n = n;
            why = zafx::maskfilter_stereo_refusal(c, mc);
        } else {
            if (!read_lengths(lengths)) return 2;
            clip = -2;
            why = zafx::maskfilter_stereo_ragged_refusal(kind, layout, mc, lengths.data(), (int64_t)lengths.size(), &clip);
        }
        if (why) std::printf("refused %lld: %s\n", (long long)clip, why);
        else std::printf("taken\n");
    }
    return 0;
}
