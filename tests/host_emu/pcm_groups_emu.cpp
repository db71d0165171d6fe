// The group cutter of zafx_execute_ragged_pcm's convert-first route (rg_pcm_groups, zafx_ragged_table.hpp) on the host: prints the groups of one batch.
//     g++ -O2 -std=c++17 -I zaf-python_amd/csrc tests/host_emu/pcm_groups_emu.cpp -o pcm_groups_emu
//     ./pcm_groups_emu budget_frames off0 len0 off1 len1 ...       (the clips' offsets and lengths in sample frames)
// Output: "groups <n>", then one line "first count lo hi" per group.  The program checks nothing itself: tests/test_pcm_ragged_host.py holds
// the properties, and runs a build of this file with -fsanitize=address,undefined on the same batches.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "zafx_ragged_table.hpp"

int main(int argc, char** argv) {
    if (argc < 2 || argc % 2 != 0) return 2;
    const long long budget = std::atoll(argv[1]);
    std::vector<int64_t> offsets, lengths;
    for (int i = 2; i + 1 < argc; i += 2) {
        offsets.push_back(std::atoll(argv[i]));
        lengths.push_back(std::atoll(argv[i + 1]));
    }
    // (n = 0: the arrays are empty and never read)
    const std::vector<zafx::RgPcmGroup> groups = zafx::rg_pcm_groups(offsets.data(), lengths.data(), (long long)offsets.size(), budget);
    std::printf("groups %zu\n", groups.size());
    for (const zafx::RgPcmGroup& g : groups) std::printf("%lld %lld %lld %lld\n", g.first, g.count, g.lo, g.hi);
    return 0;
}
