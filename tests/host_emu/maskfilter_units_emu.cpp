// Ragged batches of the mask filter on the host: the cutter (maskfilter_cut_units, zafx_units.hpp), the deal (deal_table) and a CPU model of
// k_maskfilter's RAGGED walk (zafx_maskfilter.hip) -- a clip walked unit by unit, every unit from its own record, the ZAFX_LAYOUT_FT stage
// filled per two tiles from the unit's first transform on -- in float32 as on the device.
//     g++ -O2 -std=c++17 -DZAFX_HOST_EMU -I zaf-python_amd/csrc tests/host_emu/maskfilter_units_emu.cpp -o maskfilter_units_emu
//     ./maskfilter_units_emu cut W F slots per_slot grid        lengths on standard input, one per token
//         Clip i rides with in_off 1000 + i, out_off 2 (1000 + i), mask_off 3 (1000 + i) + 1 and mask pitch 7 + i.
//         Output: one line "U in_off n_samples out_off mask_off b0 b1 mask_pitch" per unit in the order the kernel walks them, then one line
//         "D ..." of the same fields per record of deal_table(units, grid).
//     ./maskfilter_units_emu walk
//         stdin: int32 W, N, tf, pitch, F, slots, per_slot; float32 window[W], x[N], mask (FT: W/2+1 rows of `pitch`; TF: T x (W/2+1))
//         stdout: int32 n_units, float32 y[N] of the clip walked as the cutter's units, float32 y[N] of the clip walked as one unit
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
static void walk_unit(const MaskfilterUnit& rc, bool tf, int F, const std::vector<float>& win, const float* x, const float* mask, float* out) {
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
    const float *xc = x + rc.in_off, *mc = mask + rc.mask_off;
    float* oc = out + rc.out_off;
    // the two descriptors: 4 n bytes of samples; the mask up to its last frame's last bin
    const long long mask_elems = tf ? (n_blocks + 1) * (H + 1) : (long long)H * rc.mask_pitch + n_blocks + 1;
    auto sample = [&](long long s) { return s >= 0 && s < n ? xc[s] : 0.f; };
    auto mload = [&](int k, long long t) {
        if (t > n_blocks) return 0.f;   // a frame beyond the clip's last reads no mask
        const long long e = tf ? t * (H + 1) + k : (long long)k * rc.mask_pitch + t;
        return e >= 0 && e < mask_elems ? mc[e] : 0.f;
    };
    const int FS = 4 * F, q0 = rc.b0 >> 1, q1 = rc.b1 >> 1;
    std::vector<float> stage((size_t)(H + 1) * (size_t)FS);
    std::vector<float2> regs((size_t)W), buf((size_t)C::PITCH);
    std::vector<float> carry((size_t)H);
    for (int q = q0; q <= q1; ++q) {
        const int qs = q0 + (q - q0) / (2 * F) * (2 * F);
        if (!tf && q == qs)   // FT: frames 2 qs .. 2 qs + FS - 1 of every row
            for (int r = 0; r <= H; ++r)
                for (int c = 0; c < FS; ++c) stage[(size_t)r * FS + c] = mload(r, 2LL * qs + c);
        for (int p = 0; p < C::P; ++p)
            for (int i = 0; i < C::E; ++i) {
                const int k = p + i * C::P;
                const long long s = (2LL * q - 1) * H + k;
                regs[(size_t)p * C::E + i] = make_float2(sample(s) * win[(size_t)k], sample(s + H) * win[(size_t)k]);
            }
        Runner<LOG2W, LOG2E, 0>::run(regs, buf, tw.data());
        for (int k = 0; k <= H; ++k) {
            const int pk = phys_t<C::PS>(k), pn = phys_t<C::PS>((W - k) & (W - 1));
            const float ma = tf ? mload(k, 2LL * q) : stage[(size_t)k * FS + 2 * (q - qs)];
            const float mb = tf ? mload(k, 2LL * q + 1) : stage[(size_t)k * FS + 2 * (q - qs) + 1];
            float2 ck, cn;
            maskfilter_pair(buf[(size_t)pk], buf[(size_t)pn], ma, mb, ck, cn);
            buf[(size_t)pk] = center_swap(ck);
            buf[(size_t)pn] = center_swap(cn);
        }
        for (int p = 0; p < C::P; ++p) regs_read<LOG2W, LOG2E>(&regs[(size_t)p * C::E], buf.data(), p);
        Runner<LOG2W, LOG2E, 0>::run(regs, buf, tw.data());
        if (q > q0)   // block 2q - 1
            for (int k = 0; k < H; ++k) {
                const long long s = (2LL * q - 1) * H + k;
                if (s < n) oc[s] = (carry[(size_t)k] + buf[(size_t)phys_t<C::PS>(k)].y) * gain;
            }
        if (2 * q < rc.b1)   // block 2q
            for (int k = 0; k < H; ++k) {
                const long long s = 2LL * q * H + k;
                if (s < n) oc[s] = (buf[(size_t)phys_t<C::PS>(H + k)].y + buf[(size_t)phys_t<C::PS>(k)].x) * gain;
            }
        for (int k = 0; k < H; ++k) carry[(size_t)k] = buf[(size_t)phys_t<C::PS>(H + k)].x;
    }
}

static void walk(int w, const MaskfilterUnit& rc, bool tf, int F, const std::vector<float>& win, const float* x, const float* mask, float* out) {
    switch (w) {
        case 256: walk_unit<8>(rc, tf, F, win, x, mask, out); break;
        case 512: walk_unit<9>(rc, tf, F, win, x, mask, out); break;
        case 1024: walk_unit<10>(rc, tf, F, win, x, mask, out); break;
        case 2048: walk_unit<11>(rc, tf, F, win, x, mask, out); break;
        default: std::exit(3);
    }
}

static void print_unit(const char* tag, const MaskfilterUnit& u) {
    std::printf("%s %lld %lld %lld %lld %d %d %d\n", tag, u.in_off, u.n_samples, u.out_off, u.mask_off, u.b0, u.b1, u.mask_pitch);
}

static int main_cut(int argc, char** argv) {
    if (argc != 7) return 2;
    const int W = std::atoi(argv[2]), F = std::atoi(argv[3]), per_slot = std::atoi(argv[5]);
    const long long slots = std::atoll(argv[4]), grid = std::atoll(argv[6]);
    std::vector<int64_t> lengths, in, out, mo, mp;
    long long v;
    while (std::scanf("%lld", &v) == 1) lengths.push_back(v);
    for (size_t i = 0; i < lengths.size(); ++i) {
        const int64_t id = 1000 + (int64_t)i;
        in.push_back(id), out.push_back(2 * id), mo.push_back(3 * id + 1), mp.push_back(7 + (int64_t)i);
    }
    const auto units = maskfilter_cut_units(lengths.data(), in.data(), out.data(), mo.data(), mp.data(), (int64_t)lengths.size(), W, F, slots, per_slot);
    for (const auto& u : units) print_unit("U", u);
    for (const auto& u : deal_table(units, grid)) print_unit("D", u);
    return 0;
}

static int main_walk() {
    int hdr[7];
    if (fread(hdr, sizeof(int), 7, stdin) != 7) return 2;
    const int w = hdr[0], tf = hdr[2], pitch = hdr[3], F = hdr[4], slots = hdr[5], per_slot = hdr[6];
    const long long n = hdr[1];
    if (w < 2 || n < 0) return 3;
    const int64_t frames = maskfilter_frames(n, w);
    std::vector<float> win((size_t)w), x((size_t)n), mask((size_t)(tf ? frames * (w / 2 + 1) : (int64_t)(w / 2 + 1) * pitch));
    if (fread(win.data(), sizeof(float), win.size(), stdin) != win.size()) return 2;
    if (fread(x.data(), sizeof(float), x.size(), stdin) != x.size()) return 2;
    if (fread(mask.data(), sizeof(float), mask.size(), stdin) != mask.size()) return 2;
    const int64_t len = n, mp = pitch;
    const auto units = maskfilter_cut_units(&len, nullptr, nullptr, nullptr, &mp, 1, w, F, slots, per_slot);
    std::vector<float> cut((size_t)n, -1.f), whole((size_t)n, -1.f);
    for (auto it = units.rbegin(); it != units.rend(); ++it) walk(w, *it, tf != 0, F, win, x.data(), mask.data(), cut.data());   // (any order)
    const MaskfilterUnit all{0, n, 0, 0, 0, (int)center_blocks(n, w), pitch, 0};
    walk(w, all, tf != 0, F, win, x.data(), mask.data(), whole.data());
    const int n_units = (int)units.size();
    fwrite(&n_units, sizeof(int), 1, stdout);
    fwrite(cut.data(), sizeof(float), cut.size(), stdout);
    return fwrite(whole.data(), sizeof(float), whole.size(), stdout) == whole.size() ? 0 : 4;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "cut")) return main_cut(argc, argv);
    if (argc == 2 && !std::strcmp(argv[1], "walk")) return main_walk();
    return 2;
}
