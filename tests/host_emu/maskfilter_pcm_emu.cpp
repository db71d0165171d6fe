// The sample arithmetic of the PCM mask filter (zafx_maskfilter_pcm.hpp) on the host: what k_maskfilter_pcm and k_maskfilter_stereo_pcm do to
// a sample on its way in and on its way out, asked of the very functions the kernels call.
// Build: g++ -O2 -std=c++17 -DZAFX_HOST_EMU -I zaf-python_amd/csrc tests/host_emu/maskfilter_pcm_emu.cpp -o maskfilter_pcm_emu
//   maskfilter_pcm_emu q      stdin: float32 values y             stdout: int32 pcm_quantise(y) each
//   maskfilter_pcm_emu r      stdin: int32 pairs (x, q)           stdout: int32 pcm_rest(x, q) each
//   maskfilter_pcm_emu s      (no input)                          stdout: for every int16 s from -32768 up, int32 pcm_quantise(pcm_sample(s)) and
//                                                                         float32 pcm_sample(s), then int32 left and right of pcm_pack(s, -s - 1)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "zafx_maskfilter_pcm.hpp"

template <class T>
static std::vector<T> read_all() {
    std::vector<T> v;
    T buf[4096];
    size_t n;
    while ((n = std::fread(buf, sizeof(T), 4096, stdin)) > 0) v.insert(v.end(), buf, buf + n);
    return v;
}

template <class T>
static void put(T v) { std::fwrite(&v, sizeof(T), 1, stdout); }

int main(int argc, char** argv) {
    if (argc != 2 || std::strlen(argv[1]) != 1) return 2;
    switch (argv[1][0]) {
        case 'q':
            for (float y : read_all<float>()) put<int32_t>(zafx::pcm_quantise(y));
            return 0;
        case 'r': {
            const std::vector<int32_t> v = read_all<int32_t>();
            if (v.size() % 2) return 2;
            for (size_t i = 0; i < v.size(); i += 2) put<int32_t>(zafx::pcm_rest(v[i], v[i + 1]));
            return 0;
        }
        case 's':
            for (int s = -32768; s <= 32767; ++s) {
                put<int32_t>(zafx::pcm_quantise(zafx::pcm_sample(s)));
                put<float>(zafx::pcm_sample(s));
                const int d = zafx::pcm_pack(s, -s - 1);
                put<int32_t>(zafx::pcm_left(d));
                put<int32_t>(zafx::pcm_right(d));
            }
            return 0;
    }
    return 2;
}
