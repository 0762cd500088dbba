// emu_spread_segs.cpp — the rule that cuts a range of one-off tasks into spread segments (swarmkit_amd/csrc/swp_rounds.hpp
// spread_segments), the header alone, on a string of task kinds: '.' a task without preferences, 's' one with, 'm' one the spread
// kernel cannot take (cluster mounts); a digit string in front of a letter repeats it ("130." = 130 plain tasks).
// Prints one line per piece: first count spread. TEST INFRASTRUCTURE (tests/test_spread_segments_cpu.py); not product.
#include <cctype>
#include <cstdio>
#include <string>

#include "../../swarmkit_amd/csrc/swp_rounds.hpp"

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s <kinds> [j0 j1]\n", argv[0]); return 2; }
    std::string k;
    for (const char* p = argv[1]; *p;) {
        unsigned rep = 0;
        bool have = false;
        while (isdigit((unsigned char)*p)) { rep = rep * 10 + (unsigned)(*p++ - '0'); have = true; }
        if (!*p) return 2;
        k.append(have ? rep : 1u, *p++);
    }
    const uint32_t j0 = argc > 3 ? (uint32_t)atoi(argv[2]) : 0u, j1 = argc > 3 ? (uint32_t)atoi(argv[3]) : (uint32_t)k.size();
    const uint32_t n = swpdev::spread_segments(
        j0, j1, [&](uint32_t j) { return k[j] == 's' ? (int)swpdev::SPREAD_TASK : k[j] == 'm' ? (int)swpdev::SPREAD_FENCE : (int)swpdev::SPREAD_PLAIN; },
        [](uint32_t first, uint32_t count, bool spread) { printf("%u %u %d\n", first, count, spread ? 1 : 0); });
    printf("segments %u gap %u\n", n, swpdev::SPREAD_GAP);
    return 0;
}
