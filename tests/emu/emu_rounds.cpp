// emu_rounds.cpp — swarmkit_amd/csrc/swp_rounds.hpp alone (no HIP, no engine): prints what the round drivers' host rules give for
// scripted inputs; tests/test_rounds_cpu.py compares with literals recorded from the expressions the drivers used to carry themselves.
// TEST INFRASTRUCTURE around product source; no product code path uses it.
//   first n...                                  the first chunk of a stretch of n tasks
//   step rest recent cur largest forced         one replan with `rest` tasks left and the block at `cur`: "chunk block"
//   pace n largest forced (pos rounds)...       the shard drivers' use (advance): "chunk block" at the start and after every pair
//   single start end largest forced (pos rounds)...   the single engine's use (observe, then replan): the same
//   fit block base per                          r6_fit_block with lds(block) = base + per * block: the blocks probed, then the result
//   knobs classes_ok n_classes                  r6_knobs(1024, 768) from the environment: "dbg forced cap wish rows"
#include <cstdio>
#include <cstring>

#include "../../swarmkit_amd/csrc/swp_rounds.hpp"

using namespace swpdev;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const char* cmd = argv[1];
    auto u = [&](int i) { return (uint32_t)atoi(argv[i]); };
    if (!strcmp(cmd, "first")) {
        for (int i = 2; i < argc; ++i) printf("%u\n", RoundPace(u(i), 768, false).chunk);
    } else if (!strcmp(cmd, "step") && argc == 7) {
        RoundPace p(u(2), u(5), u(6) != 0);
        p.block = u(4);
        p.replan(atof(argv[3]));
        printf("%u %u\n", p.chunk, p.block);
    } else if (!strcmp(cmd, "pace") && argc >= 5) {
        RoundPace p(u(2), u(3), u(4) != 0);
        printf("%u %u\n", p.chunk, p.block);
        for (int i = 5; i + 1 < argc; i += 2) {
            p.advance(u(i), u(i + 1));
            printf("%u %u\n", p.chunk, p.block);
        }
    } else if (!strcmp(cmd, "single") && argc >= 6) {
        RoundPace p(u(3) - u(2), u(4), u(5) != 0, u(2));
        printf("%u %u\n", p.chunk, p.block);
        for (int i = 6; i + 1 < argc; i += 2) {
            const double recent = p.observe(u(i), u(i + 1));
            p.replan(recent);
            printf("%u %u\n", p.chunk, p.block);
        }
    } else if (!strcmp(cmd, "fit") && argc == 5) {
        const size_t base = (size_t)atol(argv[3]), per = (size_t)atol(argv[4]);
        const uint32_t got = r6_fit_block(u(2), [&](uint32_t bl) {
            printf("%u ", bl);
            return base + per * bl;
        });
        printf("-> %u\n", got);
    } else if (!strcmp(cmd, "knobs") && argc == 4) {
        const R6Knobs k = r6_knobs(1024, 768);
        printf("%u %d %u %d %d\n", k.dbg, k.block_forced ? 1 : 0, k.block_cap, k.task_rows, r6_task_rows(k, u(2) != 0, u(3)) ? 1 : 0);
    } else
        return 2;
    return 0;
}
