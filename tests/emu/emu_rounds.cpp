// emu_rounds.cpp — swarmkit_amd/csrc/swp_rounds.hpp alone (no HIP, no engine): prints what the round drivers' host rules give for
// scripted inputs; tests/test_rounds_cpu.py compares with literals recorded from the expressions the drivers used to carry themselves.
// TEST INFRASTRUCTURE around product source; no product code path uses it.
//   first n...                                  the first chunk of a stretch of n tasks
//   step rest recent cur largest forced         one replan with `rest` tasks left and the block at `cur`: "chunk block"
//   pace n largest forced (pos rounds)...       the shard drivers' use (advance): "chunk block" at the start and after every pair
//   single start end largest forced (pos rounds)...   the single engine's use (observe, then replan): the same
//   fit block base per                          r6_fit_block with lds(block) = base + per * block: the blocks probed, then the result
//   knobs classes_ok n_classes                  r6_knobs(1024, 768) from the environment: "dbg forced cap wish rows runs compact fused scan twins"
//   runs T tasks_in_runs                        r6_shape with the environment's knobs: "runs win cap"
//   compact allowed hint (used recent block exh crounds stops)...   CompactSwitch fed one chunk's increments after the other: "on compact"
//                                               at the start and after every tuple, then "ever 0/1"
//   scan ok fast op...                          ScanHandover: due used recent left | stretch pos end -> "scan j0 j1 chunk len" | again pos upto
//                                               end skipped | rounds (rounds went on: after_scan off) | cap chunk recent; then "scanned n"
//   drive start end largest forced runs allowed hint scan_ok scan_fast report node_local (pos rounds cuts crounds reseats skipped)...
//                                               RoundRules over a whole stretch as batch_run_impl drives it; one tuple of words per
//                                               read-back: "rounds chunk block compact ext" / "scan j0 j1", then "end pos ever e scanned n words k"
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
        printf("%u %d %u %d %d", k.dbg, k.block_forced ? 1 : 0, k.block_cap, k.task_rows, r6_task_rows(k, u(2) != 0, u(3)) ? 1 : 0);
        printf(" %d %d %d %d %d\n", k.runs, k.compact, k.compact_fused ? 1 : 0, k.scan ? 1 : 0, k.twins ? 1 : 0);
    } else if (!strcmp(cmd, "runs") && argc == 4) {
        const R6Shape s = r6_shape(r6_knobs(1408, 1408), u(3), u(2));   // (the kernel's largest block: the cap of 768 for runs shows)
        printf("%d %u %u\n", s.runs ? 1 : 0, s.win, s.cap);
    } else if (!strcmp(cmd, "compact") && argc >= 4) {
        CompactSwitch c(u(2) != 0, r6_knobs(1024, 768), u(3) != 0);
        R6Words w{};
        printf("%d %u\n", c.on ? 1 : 0, c.compact());
        for (int i = 4; i + 5 < argc; i += 6) {
            w.cuts += u(i + 3);
            w.crounds += u(i + 4);
            w.reseats += u(i + 5);
            c.feed(u(i), atof(argv[i + 1]), u(i + 2), w);
            printf("%d %u\n", c.on ? 1 : 0, c.compact());
        }
        printf("ever %d\n", c.ever ? 1 : 0);
    } else if (!strcmp(cmd, "scan") && argc >= 4) {
        ScanHandover s(u(2) != 0, u(3) != 0);
        for (int i = 4; i < argc;) {
            const char* op = argv[i];
            if (!strcmp(op, "due") && i + 3 < argc) {
                printf("due %d\n", s.due(u(i + 1), atof(argv[i + 2]), u(i + 3)) ? 1 : 0);
                i += 4;
            } else if (!strcmp(op, "stretch") && i + 2 < argc) {
                const uint32_t pos = u(i + 1), upto = s.upto(pos, u(i + 2)), chunk = s.took(pos, upto);
                printf("scan %u %u %u %u\n", pos, upto, chunk, s.len);
                i += 3;
            } else if (!strcmp(op, "again") && i + 4 < argc) {
                printf("again %d\n", s.again(u(i + 1), u(i + 2), u(i + 3), u(i + 4)) ? 1 : 0);
                i += 5;
            } else if (!strcmp(op, "rounds")) {
                s.after_scan = false;
                i += 1;
            } else if (!strcmp(op, "cap") && i + 2 < argc) {
                printf("cap %u\n", s.cap_chunk(u(i + 1), atof(argv[i + 2])));
                i += 3;
            } else
                return 2;
        }
        printf("scanned %u\n", s.scanned);
    } else if (!strcmp(cmd, "drive") && argc >= 13) {
        const uint32_t start = u(2), end = u(3);
        const R6Knobs k = r6_knobs(1024, 768);
        RoundRules rules{RoundPace(end - start, u(4), u(5) != 0, start), CompactSwitch(u(7) != 0, k, u(8) != 0), ScanHandover(u(9) != 0, u(10) != 0), u(6) == 0};
        const bool report = u(11) != 0, node_local = u(12) != 0;
        int wi = 13;
        R6Words w{};
        auto read = [&]() {
            if (wi + 5 >= argc) {
                printf("out of words\n");
                exit(3);
            }
            w = R6Words{u(wi), u(wi + 1), u(wi + 2), u(wi + 3), u(wi + 4), u(wi + 5)};
            wi += 6;
        };
        while (rules.pace.pos < rules.pace.end) {
            printf("rounds %u %u %u %s\n", rules.pace.chunk, rules.pace.block, rules.cpt.compact(), rules.ext() ? "on" : "off");
            read();
            if (w.pos <= rules.pace.pos) {
                printf("no progress\n");
                return 4;
            }
            uint32_t used;
            double recent;
            if (!rules.after_rounds(w, &used, &recent)) continue;
            for (bool again = true; again;) {
                const uint32_t upto = rules.scan_upto();
                printf("scan %u %u\n", rules.pace.pos, upto);
                const bool looks = rules.scan.looks(node_local, upto, end, report);
                if (looks) read();
                again = rules.after_scan(upto, looks ? &w : nullptr);
            }
        }
        printf("end %u ever %d scanned %u words %d\n", rules.pace.pos, rules.cpt.ever ? 1 : 0, rules.scan.scanned, (wi - 13) / 6);
    } else
        return 2;
    return 0;
}
