// emu_rounds_ring.cpp — the host rule of the block resolver's ring rounds (swarmkit_amd/csrc/swp_rounds.hpp: r6_ring, r6_ring_block,
// r6_ring_stream_every, RoundRules::ring / block) alone, no HIP and no engine: prints what the rules give for scripted inputs;
// tests/test_rounds_ring_cpu.py compares with literals worked out from the rule's text. The knobs come from the environment, as the
// driver reads them. TEST INFRASTRUCTURE around product source; no product code path uses it.
//   ring ext_on mounts single n_words left flat_block        r6_ring: "0" / "1"
//   block asked ring_block_max                               r6_ring_block
//   every every flat_block ring_block                        r6_ring_stream_every
//   drive start end flat ring_block n_words ext_ok (pos rounds)...
//       RoundRules over a stretch as run_stretch drives it (no compact index, no scan resolver): "ring block ext chunk" in front of every
//       chunk, the words of a read-back per pair
#include <cstdio>
#include <cstring>

#include "../../swarmkit_amd/csrc/swp_rounds.hpp"

using namespace swpdev;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const char* cmd = argv[1];
    auto u = [&](int i) { return (uint32_t)atoi(argv[i]); };
    const R6Knobs k = r6_knobs(2048, 2048);
    if (!strcmp(cmd, "ring") && argc == 8) {
        printf("%d\n", r6_ring(k, u(2) != 0, u(3) != 0, u(4) != 0, u(5), u(6), u(7)) ? 1 : 0);
    } else if (!strcmp(cmd, "block") && argc == 4) {
        printf("%u\n", r6_ring_block(k, u(2), u(3)));
    } else if (!strcmp(cmd, "every") && argc == 5) {
        printf("%u\n", r6_ring_stream_every(u(2), u(3), u(4)));
    } else if (!strcmp(cmd, "drive") && argc >= 8) {
        const uint32_t start = u(2), end = u(3), flat = u(4), rb = u(5), n_words = u(6);
        const bool ext_ok = u(7) != 0;
        const bool may = rb != 0 && r6_ring(k, ext_ok, false, true, n_words, end - start, flat);
        RoundRules rules{RoundPace(end - start, may ? rb : flat, k.block_forced, start), CompactSwitch(false, k, false), ScanHandover(false, false), ext_ok};
        if (may) {
            rules.flat = flat;
            rules.n_words = n_words;
            rules.ring_knobs = k;
        }
        printf("%d %u %d %u\n", rules.ring() ? 1 : 0, rules.block(), rules.ext() ? 1 : 0, rules.pace.chunk);
        R6Words w{};
        for (int i = 8; i + 1 < argc; i += 2) {
            w.pos = u(i);
            w.rounds = u(i + 1);
            uint32_t used;
            double recent;
            rules.after_rounds(w, &used, &recent);
            printf("%d %u %d %u\n", rules.ring() ? 1 : 0, rules.block(), rules.ext() ? 1 : 0, rules.pace.chunk);
        }
    } else
        return 2;
    return 0;
}
