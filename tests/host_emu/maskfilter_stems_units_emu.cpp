// Ragged batches of the mask filter's stems on the host: the cutter (maskfilter_cut_units, zafx_units.hpp) under the stems' workgroup slots and a
// CPU model of the RAGGED walk of k_maskfilter_stems (zafx_maskfilter_stems.hip) -- a clip walked unit by unit, every unit from its own record:
// the samples at x + in_off, stem s's mask (ZAFX_LAYOUT_TF, (n_blocks + 1) (H + 1) elements, read through a range check of its own) at
// mask + mask_off + s (n_blocks + 1) (H + 1), stem s's output at out + out_off + s n_samples, the rest behind the last stem -- in float32 as on
// the device: one forward transform per packed pair of frames, then per stem the mask, the inverse and the overlap-add with the stem's carry.
//     g++ -O2 -std=c++17 -DZAFX_HOST_EMU -I zaf-python_amd/csrc tests/host_emu/maskfilter_stems_units_emu.cpp -o maskfilter_stems_units_emu
//     ./maskfilter_stems_units_emu cut W F slots per_slot n_stems rest        lengths on standard input, one per token
//         The clips, their masks and their output blocks lie back to back (the layout of zafx_plan_stems_ragged_layout).
//         Output: one line "U clip in_off n_samples out_off mask_off b0 b1" per unit in the order the kernel walks them.
//     ./maskfilter_stems_units_emu walk
//         stdin: int32 W, N, S, rest, F, slots, per_slot; float32 window[W], x[N], mask[S][T][W/2+1] (T = ceil(N / (W/2)) + 1)
//         stdout: int32 n_units, float32 y[S + rest][N] of the clip walked as the cutter's units, the same of the clip walked as one unit.
//         Both walks run inside larger arrays: the clip, its masks and its block start at elements 3, 5 and 7 and end with their arrays.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "zafx_maskfilter.hpp"
#include "zafx_twiddle.hpp"
#include "zafx_units.hpp"
#include "fft_runner.hpp"

using namespace zafx;

// One unit of the table, as the kernel walks it: x, mask and out are the whole arrays, the record places the clip in them.
template <int LOG2W>
static void walk_unit(const MaskfilterUnit& rc, int stems, bool rest, const std::vector<float>& win, const float* x, const float* mask, float* out) {
    constexpr int LOG2E = maskfilter_log2e(LOG2W);
    using C = FftCfg<LOG2W, LOG2E>;
    constexpr int W = C::N, H = W / 2;
    if (rc.b1 <= rc.b0) return;   // a value-initialised record
    const auto twv = build_pass_twiddles(LOG2W, LOG2E);
    std::vector<float2> tw(twv.size() + 1);
    for (size_t i = 0; i < twv.size(); ++i) tw[i] = make_float2(twv[i].re, twv[i].im);
    double g = 0;
    for (int i = 0; i < W; i += H) g += (double)win[(size_t)i];
    const float gain = 1.f / ((float)W * (float)g);
    const long long n = rc.n_samples, n_blocks = (n + H - 1) / H;
    const long long mask_clip = (n_blocks + 1) * (H + 1);   // a stem's mask, and the range of its descriptor
    const float* const xc = x + rc.in_off;
    const float* const mc = mask + rc.mask_off;
    float* const oc = out + rc.out_off;
    auto sample = [&](long long s) { return s >= 0 && s < n ? xc[s] : 0.f; };
    auto mload = [&](int st, int k, long long t) {
        if (t > n_blocks) return 0.f;   // a frame beyond the clip's last reads no mask
        const long long e = t * (H + 1) + k;
        return e >= 0 && e < mask_clip ? mc[(long long)st * mask_clip + e] : 0.f;
    };
    const int q0 = rc.b0 >> 1, q1 = rc.b1 >> 1;
    std::vector<float2> regs((size_t)W), buf((size_t)C::PITCH), spec((size_t)C::PITCH);
    std::vector<float> carry((size_t)stems * H), raw((size_t)W);
    for (int q = q0; q <= q1; ++q) {
        const bool writes_odd = q > q0, writes_even = 2 * q < rc.b1;
        for (int p = 0; p < C::P; ++p)
            for (int i = 0; i < C::E; ++i) {
                const int k = p + i * C::P;
                const long long s = (2LL * q - 1) * H + k;
                regs[(size_t)p * C::E + i] = make_float2(sample(s) * win[(size_t)k], sample(s + H) * win[(size_t)k]);
                raw[(size_t)k] = sample(s);   // the inputs of blocks 2q - 1 (k < H) and 2q
            }
        Runner<LOG2W, LOG2E, 0>::run(regs, buf, tw.data());
        spec = buf;   // the spectrum, kept through the stems
        for (int st = 0; st < stems; ++st) {
            float* const y = oc + (long long)st * n;
            float* const cr = carry.data() + (size_t)st * H;
            for (int k = 0; k <= H; ++k) {
                const int pk = phys_t<C::PS>(k), pn = phys_t<C::PS>((W - k) & (W - 1));
                float2 ck, cn;
                maskfilter_pair(spec[(size_t)pk], spec[(size_t)pn], mload(st, k, 2LL * q), mload(st, k, 2LL * q + 1), ck, cn);
                buf[(size_t)pk] = center_swap(ck);
                buf[(size_t)pn] = center_swap(cn);
            }
            for (int p = 0; p < C::P; ++p) regs_read<LOG2W, LOG2E>(&regs[(size_t)p * C::E], buf.data(), p);
            Runner<LOG2W, LOG2E, 0>::run(regs, buf, tw.data());
            if (writes_odd)   // block 2q - 1
                for (int k = 0; k < H; ++k) {
                    const long long s = (2LL * q - 1) * H + k;
                    if (s < n) {
                        y[s] = (cr[k] + buf[(size_t)phys_t<C::PS>(k)].y) * gain;
                        raw[(size_t)k] = raw[(size_t)k] - y[s];
                    }
                }
            if (writes_even)   // block 2q
                for (int k = 0; k < H; ++k) {
                    const long long s = 2LL * q * H + k;
                    if (s < n) {
                        y[s] = (buf[(size_t)phys_t<C::PS>(H + k)].y + buf[(size_t)phys_t<C::PS>(k)].x) * gain;
                        raw[(size_t)(H + k)] = raw[(size_t)(H + k)] - y[s];
                    }
                }
            for (int k = 0; k < H; ++k) cr[k] = buf[(size_t)phys_t<C::PS>(H + k)].x;
        }
        if (rest) {
            float* const r = oc + (long long)stems * n;
            for (int k = 0; k < W; ++k) {
                const long long s = (2LL * q - 1) * H + k;
                if (s >= 0 && s < n && (k < H ? writes_odd : writes_even)) r[s] = raw[(size_t)k];
            }
        }
    }
}

static void walk(int w, const MaskfilterUnit& rc, int stems, bool rest, const std::vector<float>& win, const float* x, const float* mask, float* out) {
    switch (w) {
        case 256: walk_unit<8>(rc, stems, rest, win, x, mask, out); break;
        case 512: walk_unit<9>(rc, stems, rest, win, x, mask, out); break;
        case 1024: walk_unit<10>(rc, stems, rest, win, x, mask, out); break;
        case 2048: walk_unit<11>(rc, stems, rest, win, x, mask, out); break;
        default: std::exit(3);
    }
}

static int main_cut(int argc, char** argv) {
    if (argc != 8) return 2;
    const int W = std::atoi(argv[2]), F = std::atoi(argv[3]), per_slot = std::atoi(argv[5]), stems = std::atoi(argv[6]), rest = std::atoi(argv[7]);
    const long long slots = std::atoll(argv[4]);
    std::vector<int64_t> lengths, in, out, mo;
    long long v, at_in = 0, at_out = 0, at_mask = 0;
    while (std::scanf("%lld", &v) == 1) {
        lengths.push_back(v), in.push_back(at_in), out.push_back(at_out), mo.push_back(at_mask);
        at_in += v, at_out += (stems + (rest ? 1 : 0)) * v, at_mask += (long long)stems * maskfilter_frames(v, W) * (W / 2 + 1);
    }
    const auto units = maskfilter_cut_units(lengths.data(), in.data(), out.data(), mo.data(), nullptr, (int64_t)lengths.size(), W, F, slots, per_slot);
    for (const auto& u : units) {
        size_t clip = 0;
        while (!(in[clip] == u.in_off && lengths[clip] == u.n_samples && out[clip] == u.out_off && mo[clip] == u.mask_off)) ++clip;   // (a clip of length 0 shares its in_off)
        std::printf("U %zu %lld %lld %lld %lld %d %d\n", clip, u.in_off, u.n_samples, u.out_off, u.mask_off, u.b0, u.b1);
    }
    return 0;
}

static int main_walk() {
    int hdr[7];
    if (fread(hdr, sizeof(int), 7, stdin) != 7) return 2;
    const int w = hdr[0], stems = hdr[2], F = hdr[4], slots = hdr[5], per_slot = hdr[6];
    const bool rest = hdr[3] != 0;
    const long long n = hdr[1];
    if (w < 2 || n < 0 || stems < 1 || stems > 8) return 3;
    const int64_t frames = maskfilter_frames(n, w), in_off = 3, mask_off = 5, out_off = 7;
    const size_t mask_n = (size_t)stems * (size_t)frames * (size_t)(w / 2 + 1), out_n = (size_t)(stems + (rest ? 1 : 0)) * (size_t)n;
    // the arrays end with the clip, its masks and its block: a read or a write behind them is one behind the allocation
    std::vector<float> win((size_t)w), x((size_t)(in_off + n), -7.f), mask((size_t)mask_off + mask_n, -7.f);
    if (fread(win.data(), sizeof(float), win.size(), stdin) != win.size()) return 2;
    if (fread(x.data() + in_off, sizeof(float), (size_t)n, stdin) != (size_t)n) return 2;
    if (fread(mask.data() + mask_off, sizeof(float), mask_n, stdin) != mask_n) return 2;
    const int64_t len = n;
    const auto units = maskfilter_cut_units(&len, &in_off, &out_off, &mask_off, nullptr, 1, w, F, slots, per_slot);
    std::vector<float> cut((size_t)out_off + out_n, -1.f), whole((size_t)out_off + out_n, -1.f);
    for (auto it = units.rbegin(); it != units.rend(); ++it) walk(w, *it, stems, rest, win, x.data(), mask.data(), cut.data());   // (any order)
    const MaskfilterUnit all{in_off, n, out_off, mask_off, 0, (int)center_blocks(n, w), 0, 0};
    walk(w, all, stems, rest, win, x.data(), mask.data(), whole.data());
    for (int64_t i = 0; i < out_off; ++i)
        if (cut[(size_t)i] != -1.f || whole[(size_t)i] != -1.f) return 5;   // written in front of the block
    const int n_units = (int)units.size();
    fwrite(&n_units, sizeof(int), 1, stdout);
    fwrite(cut.data() + out_off, sizeof(float), out_n, stdout);
    return fwrite(whole.data() + out_off, sizeof(float), out_n, stdout) == out_n ? 0 : 4;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "cut")) return main_cut(argc, argv);
    if (argc == 2 && !std::strcmp(argv[1], "walk")) return main_walk();
    return 2;
}
