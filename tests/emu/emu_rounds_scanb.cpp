// emu_rounds_scanb.cpp — the single engine's scan loop (swp_engine.hip run_stretch) over a CONDITIONAL hand-over, restated around
// swarmkit_amd/csrc/swp_rounds.hpp alone with the launches replaced by prints and the device by a script: rounds that decide one task
// each; probes that answer the unions given on the command line, in order (the last one repeats); a stretch is taken by the batched
// instance when its union has at most <batched_max> nodes, and then answers <skipped_permille> thousandths of its tasks without a look.
// What it pins: behind a batched compact stretch the words are read (looks' stretch_fast), `again` follows with the next stretch behind
// a probe of its own, a refusal there applies the hold. TEST INFRASTRUCTURE (tests/test_rounds_scanb_cpu.py); not product.
//
//   emu_rounds_scanb <T> <batched_max> <skipped_permille> <union> [<union> ...]
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../swarmkit_amd/csrc/swp_rounds.hpp"

using namespace swpdev;

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    const uint32_t T = (uint32_t)atoi(argv[1]), batched_max = (uint32_t)atoi(argv[2]), permille = (uint32_t)atoi(argv[3]);
    std::vector<uint32_t> unions;
    for (int i = 4; i < argc; ++i) unions.push_back((uint32_t)atoi(argv[i]));
    size_t next_union = 0;
    R6Knobs knobs;
    RoundRules rules{RoundPace(T, 768, false, 0), CompactSwitch(false, knobs, false), ScanHandover::conditional(true, 4096), true};
    R6Words w{0, 0, 0, 0, 0, 0};   // the device's control block
    int chunks = 0;
    while (rules.pace.pos < T && chunks < 6) {
        ++chunks;
        const uint32_t n = std::min<uint32_t>(rules.pace.chunk, T - w.pos);   // a chunk of rounds: one task each
        w.pos += n;
        w.rounds += n;
        uint32_t used;
        double recent;
        bool to_scan = rules.after_rounds(w, &used, &recent);
        printf("rounds %u pos %u held %d scan %d\n", used, rules.pace.pos, rules.scan.held(rules.pace.pos) ? 1 : 0, to_scan ? 1 : 0);
        while (to_scan) {
            uint32_t upto = rules.scan_upto(), union_nodes = 0;
            for (int attempt = 0; attempt < 2; ++attempt) {
                ++rules.scan.probes;
                union_nodes = unions[std::min(next_union++, unions.size() - 1)];
                printf("probe %u %u union %u\n", rules.pace.pos, upto, union_nodes);
                const uint32_t shorter = rules.scan.shorter(rules.pace.pos, upto);
                if (rules.scan.fits(union_nodes) || shorter >= upto) break;
                if (attempt == 0) upto = shorter;
            }
            if (!rules.scan.fits(union_nodes)) {
                rules.scan_refused(recent);
                printf("refused at %u hold_until %u hold %u chunk %u\n", rules.pace.pos, rules.scan.hold_until, rules.scan.hold, rules.pace.chunk);
                break;
            }
            const bool batched = union_nodes <= batched_max;
            if (batched) w.scan_skipped += (uint32_t)((uint64_t)(upto - rules.pace.pos) * permille / 1000u);
            const bool looks = rules.scan.looks(true, upto, T, false, batched);
            const uint32_t from = rules.pace.pos;
            w.pos = upto;
            to_scan = rules.after_scan(upto, looks ? &w : nullptr);
            printf("stretch %u %u batched %d looks %d again %d chunk %u\n", from, upto, batched ? 1 : 0, looks ? 1 : 0, to_scan ? 1 : 0, rules.pace.chunk);
        }
    }
    printf("probes %u refusals %u scanned %u\n", rules.scan.probes, rules.scan.refusals, rules.scan.scanned);
    return 0;
}
