// The claim logic of k_stft_ft16's DYN form (claim_len / claim_first / claim_finish, zafx_fft.hpp) walked on the host: G workgroups, each
// with two tiles claimed ahead as in the kernel, stepped in a pseudo-random order; the eight counters are plain ints (one "workgroup" moves
// at a time).  Prints "ok" when, for every (tiles, grid) pair, every tile index was handed out exactly once, every workgroup left, the queues
// are the ranges xcd_order gives the XCDs, and no counter was touched after the last workgroup left.
//     g++ -O2 -std=c++17 -DZAFX_HOST_EMU -I zaf-python_amd/csrc tests/host_emu/claim_emu.cpp -o claim_emu && ./claim_emu
#include <cstdio>
#include <vector>

#include "zafx_fft.hpp"

using namespace zafx;

struct Wg {
    int home, q, cur, nxt;
    bool live, left;
};

static int xcd_order_host(int v, int total) {   // (xcd_order of zafx_fft.hpp, device only there)
    const int x = v & 7, q = total >> 3, r = total & 7;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (v >> 3);
}

static bool walk(int total, int grid, unsigned seed) {
    int counters[kClaimQueues + 1] = {};
    auto draw = [&](int q) { return counters[q]++; };
    std::vector<int> hits((size_t)total, 0);
    std::vector<Wg> wg((size_t)grid);
    // the queues partition [0, total) as xcd_order does
    for (int x = 0, at = 0; x < kClaimQueues; ++x) {
        if (claim_first(x, total) != at || claim_len(x, total) < 0) return false;
        for (int j = 0; j < claim_len(x, total); ++j)
            if (xcd_order_host(x + 8 * j, total) != at + j) return false;
        at += claim_len(x, total);
        if (x == kClaimQueues - 1 && at != total) return false;
    }
    for (int b = 0; b < grid; ++b) {   // the prologue: two tiles
        Wg& w = wg[(size_t)b];
        w.home = w.q = b & (kClaimQueues - 1);
        w.left = false;
        w.cur = claim_finish(w.q, w.home, total, draw(w.q), draw);
        w.nxt = w.cur >= 0 ? claim_finish(w.q, w.home, total, draw(w.q), draw) : -1;
        w.live = w.nxt >= 0;
    }
    int running = grid;
    unsigned s = seed * 2654435761u + 12345u;
    while (running > 0) {
        s = s * 1664525u + 1013904223u;
        Wg& w = wg[(size_t)((s >> 8) % (unsigned)grid)];
        if (w.left) continue;
        if (w.cur < 0) {   // leaving: the ninth counter; the last one zeroes all
            w.left = true;
            --running;
            if (counters[kClaimQueues]++ == grid - 1)
                for (int& c : counters) c = 0;
            continue;
        }
        if (w.cur >= total) return false;
        ++hits[(size_t)w.cur];   // the tile is stored whole
        const int c = w.live ? claim_finish(w.q, w.home, total, draw(w.q), draw) : -1;   // the tile after next
        w.live = c >= 0;
        w.cur = w.nxt;
        w.nxt = c;
    }
    for (int h : hits)
        if (h != 1) return false;
    for (int c : counters)
        if (c != 0) return false;
    return true;
}

int main() {
    const int totals[] = {0, 1, 7, 8, 9, 81, 255, 256, 257, 511, 567, 1728, 27647, 27648};
    const int grids[] = {1, 3, 7, 8, 81, 255, 256, 257, 304, 512};
    for (int total : totals)
        for (int grid : grids)
            for (unsigned seed = 0; seed < 3; ++seed)
                if (!walk(total, grid, seed)) {
                    std::printf("FAILED tiles %d grid %d seed %u\n", total, grid, seed);
                    return 1;
                }
    std::printf("ok\n");
    return 0;
}
