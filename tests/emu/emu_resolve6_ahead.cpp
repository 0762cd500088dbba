// emu_resolve6_ahead.cpp — the matcher's entries requested ahead of the cursor (swp_resolve6.hpp, r6_commit_t, R6_SEAT_AHEAD) against
// the same source built with the switch off: ONE program of two objects, this file compiled with -DAHEAD_V=0 and with -DAHEAD_V=1.
// Each object holds the product headers, the model and the two drivers emu_resolve6_heads.cpp / emu_resolve7.cpp (their `main` renamed,
// their checks against the sequential model and their exit codes as they are) in a namespace of its own, with R6_SEAT_AHEAD = AHEAD_V.
// The kernel's R6_REACH hook counts the paths a run of the matcher comes across and records every round's outcome (accepted tasks,
// reason of the cut, seating steps, stops, the pick slots of the accepted tasks, the control block's counters). The program runs every
// case below under both builds from the same state and the same wave order, requires both to agree with the model (the drivers' exit
// code 0), the two records to be EQUAL, and every path a case is there for to have been reached — by the build with the switch on.
// TEST INFRASTRUCTURE (tests/test_emu_resolve6_ahead.py); not product. Stand-alone: it is also built with -fsanitize=address,undefined.
//
//   emu_resolve6_ahead            every case
//   emu_resolve6_ahead <name>     one case
//   emu_resolve6_ahead list       the names
#include "wv_emu.hpp"
#include <unistd.h>

#include <algorithm>
#include <map>
#include <random>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#ifndef AHEAD_V
#error "compile with -DAHEAD_V=0 and with -DAHEAD_V=1, link the two objects"
#endif

enum {
    R6R_ROUND, R6R_THREE_STOPS, R6R_IDLE_LANES, R6R_SECOND_STEP, R6R_AT_NENT, R6R_CLAMPED, R6R_ONE_ENTRY, R6R_SHORT_GROUP, R6R_FIRST_EXC,
    R6R_UNCOUNTED, R6R_MOUNTS, R6R_BEHIND_RUNS, R6R_COMPACT, R6R_R7, R6R_N
};
struct AheadRound {
    uint32_t pos, acc, why, seat_steps, reseats;
    uint32_t rounds, total_reseats, cut_exhausted, cut_window, cut_exception, cut_uncounted;   // the control block behind the round
    std::vector<uint32_t> node, idx, aux;   // the pick slots of the accepted tasks
    bool operator==(const AheadRound& o) const {
        return pos == o.pos && acc == o.acc && why == o.why && seat_steps == o.seat_steps && reseats == o.reseats && rounds == o.rounds && total_reseats == o.total_reseats &&
               cut_exhausted == o.cut_exhausted && cut_window == o.cut_window && cut_exception == o.cut_exception && cut_uncounted == o.cut_uncounted && node == o.node && idx == o.idx &&
               aux == o.aux;
    }
};
struct AheadResult {
    int rc = -1;
    std::vector<AheadRound> rounds;
    unsigned long long reach[R6R_N] = {};
};

#define AHEAD_CAT2(a, b) a##b
#define AHEAD_CAT(a, b) AHEAD_CAT2(a, b)
#define AHEAD_NS AHEAD_CAT(ahead_build_, AHEAD_V)
#define R6_SEAT_AHEAD AHEAD_V

namespace AHEAD_NS {
static AheadResult* cur_result = nullptr;
static bool r6_reach_round(const void* blk, uint32_t pos, uint32_t acc, uint32_t why, uint32_t seat_steps, uint32_t reseats, const uint32_t* pk_node, const uint32_t* pk_idx, const uint32_t* pk_aux);
#define R6_REACH(what, cond)                        \
    do {                                            \
        if (cond) ++cur_result->reach[what];        \
    } while (0)

namespace swpdev { using namespace ::swpdev; }   // (swp_types.hpp came with wv_emu.hpp: shared; everything behind it is this build's own)
#define SWP_R6_KERNELS
#include "../../swarmkit_amd/csrc/swp_resolve6.hpp"
#include "../../swarmkit_amd/csrc/swp_resolve7.hpp"

#include "emu_model.hpp"

static bool r6_reach_round(const void* blk, uint32_t pos, uint32_t acc, uint32_t why, uint32_t seat_steps, uint32_t reseats, const uint32_t* pk_node, const uint32_t* pk_idx, const uint32_t* pk_aux) {
    const swpdev::Blk6* b = static_cast<const swpdev::Blk6*>(blk);
    AheadRound r{pos, acc, why, seat_steps, reseats, b->rounds, b->reseats, b->cut_exhausted, b->cut_window, b->cut_exception, b->cut_uncounted, {}, {}, {}};
    r.node.assign(pk_node, pk_node + acc);
    r.idx.assign(pk_idx, pk_idx + acc);
    r.aux.assign(pk_aux, pk_aux + acc);
    cur_result->rounds.push_back(std::move(r));
    return true;
}

namespace d6 {
#define main emu_main
#include "emu_resolve6_heads.cpp"
#undef main
}   // namespace d6
namespace d7 {
#define main emu_main
#include "emu_resolve7.cpp"
#undef main
}   // namespace d7
}   // namespace AHEAD_NS

AheadResult AHEAD_CAT(ahead_run_, AHEAD_V)(bool r7, const std::vector<std::string>& args) {
    AheadResult res;
    AHEAD_NS::cur_result = &res;
    std::vector<char*> argv;
    std::string prog = r7 ? "emu_resolve7" : "emu_resolve6_heads";
    argv.push_back(prog.data());
    std::vector<std::string> own = args;
    for (std::string& s : own) argv.push_back(s.data());
    argv.push_back(nullptr);
    emu::launch_counter() = 0;   // (the wave order of a launch is drawn from the seed and this counter: the same for both builds)
    res.rc = r7 ? AHEAD_NS::d7::emu_main((int)own.size() + 1, argv.data()) : AHEAD_NS::d6::emu_main((int)own.size() + 1, argv.data());
    AHEAD_NS::cur_result = nullptr;
    return res;
}

#if AHEAD_V == 1
AheadResult ahead_run_0(bool r7, const std::vector<std::string>& args);

struct Case {
    const char* name;
    bool r7;
    const char* lvl_mode;             // EMU_LVL_MODE of the model's node levels (nullptr: its default)
    std::vector<std::string> args;    // the driver's: seed N T S block order features [shards] options (at most 256 nodes and 400 tasks)
    std::vector<int> need;            // the paths the case is there for
};

static const char* reach_name[R6R_N] = {"rounds", "group_with_3_stops", "stop_with_idle_lanes", "second_seating_step", "cursor_at_list_end", "read_clamped_at_window_end", "window_of_one_entry",
                                        "group_below_64_tasks", "first_task_from_exception_list", "uncounted_task", "mounts_task", "group_behind_run_prefix", "compact_index_round", "r7_instance"};

int main(int argc, char** argv) {
    // Blocks of 256 tasks (four groups; 64 and 320 once) on 256 nodes or fewer: the model's default levels and mode 5 leave a half-word few
    // candidates, so lists run dry all the time (stops, cursors at their end); `P` turns the kernel's section timers on.
    const std::vector<Case> cases = {
        {"stops_rr", false, nullptr, {"7", "256", "400", "40", "256", "0", "0", "P"}, {R6R_THREE_STOPS, R6R_IDLE_LANES, R6R_AT_NENT, R6R_SHORT_GROUP}},
        {"stops_lvl5", false, "5", {"11", "256", "400", "40", "320", "0", "0"}, {R6R_THREE_STOPS, R6R_IDLE_LANES}},
        {"window_3_entries", false, nullptr, {"5", "256", "400", "40", "256", "0", "0", "W3"}, {R6R_CLAMPED, R6R_AT_NENT}},
        {"window_1_entry", false, nullptr, {"5", "256", "400", "40", "256", "0", "0", "W1"}, {R6R_ONE_ENTRY, R6R_CLAMPED}},
        {"features_2_blocks_of_64", false, nullptr, {"3", "64", "200", "8", "64", "2", "2"}, {R6R_FIRST_EXC}},
        {"features_2_blocks_of_256", false, nullptr, {"9", "256", "400", "12", "256", "2", "2", "P"}, {R6R_UNCOUNTED, R6R_IDLE_LANES}},
        {"mounts", false, nullptr, {"34", "256", "400", "30", "256", "0", "4", "m10", "a"}, {R6R_MOUNTS}},
        {"runs_major", false, "0", {"103", "256", "400", "4", "256", "1", "0", "P"}, {R6R_BEHIND_RUNS, R6R_SECOND_STEP}},
        {"runs_major_win32", false, "0", {"103", "256", "400", "4", "256", "1", "0", "L32"}, {R6R_BEHIND_RUNS}},
        {"compact", false, "5", {"12", "256", "400", "40", "256", "0", "0", "c"}, {R6R_COMPACT}},
        {"compact_fused", false, "5", {"13", "256", "400", "40", "256", "0", "0", "f"}, {R6R_COMPACT}},
        {"r7_3_shards", true, nullptr, {"21", "256", "400", "40", "256", "0", "0", "3"}, {R6R_R7, R6R_THREE_STOPS}},
        {"r7_mounts", true, nullptr, {"22", "256", "300", "20", "256", "0", "4", "2", "m10"}, {R6R_R7, R6R_MOUNTS}},
    };
    if (argc > 1 && std::string(argv[1]) == "list") {
        for (const Case& c : cases) printf("%s\n", c.name);
        return 0;
    }
    int bad = 0, ran = 0;
    unsigned long long total[R6R_N] = {};
    for (const Case& c : cases) {
        if (argc > 1 && std::string(argv[1]) != c.name) continue;
        ++ran;
        if (c.lvl_mode) setenv("EMU_LVL_MODE", c.lvl_mode, 1);
        else unsetenv("EMU_LVL_MODE");
        const AheadResult off = ahead_run_0(c.r7, c.args), on = ahead_run_1(c.r7, c.args);
        bool ok = true;
        if (off.rc != 0 || on.rc != 0) { fprintf(stderr, "case %s: against the model: switch off rc %d, switch on rc %d\n", c.name, off.rc, on.rc); ok = false; }
        if (off.rounds.size() != on.rounds.size()) { fprintf(stderr, "case %s: %zu rounds with the switch off, %zu with it on\n", c.name, off.rounds.size(), on.rounds.size()); ok = false; }
        for (size_t k = 0; ok && k < on.rounds.size(); ++k)
            if (!(off.rounds[k] == on.rounds[k])) {
                const AheadRound &x = off.rounds[k], &y = on.rounds[k];
                fprintf(stderr, "case %s: launch %zu differs: off {pos %u acc %u why %u seat_steps %u stops %u} on {pos %u acc %u why %u seat_steps %u stops %u}%s\n", c.name, k, x.pos, x.acc, x.why,
                        x.seat_steps, x.reseats, y.pos, y.acc, y.why, y.seat_steps, y.reseats, x.node == y.node ? "" : " — the picks differ");
                ok = false;
            }
        for (int q = 0; q < R6R_N; ++q) {
            total[q] += on.reach[q];
            if (q != R6R_CLAMPED && off.reach[q] != on.reach[q]) { fprintf(stderr, "case %s: path %s met %llu times with the switch off, %llu with it on\n", c.name, reach_name[q], off.reach[q], on.reach[q]); ok = false; }
        }
        if (on.rounds.empty()) { fprintf(stderr, "case %s: no round recorded\n", c.name); ok = false; }
        for (int q : c.need)
            if (on.reach[q] == 0) { fprintf(stderr, "case %s: never reached: %s\n", c.name, reach_name[q]); ok = false; }
        printf("ahead case %s: %s launches=%zu", c.name, ok ? "OK" : "FAIL", on.rounds.size());
        for (int q = 1; q < R6R_N; ++q) printf(" %s=%llu", reach_name[q], on.reach[q]);
        printf("\n");
        fflush(stdout);
        if (!ok) ++bad;
    }
    if (!ran) { fprintf(stderr, "no such case\n"); return 2; }
    if (argc == 1)
        for (int q = 0; q < R6R_N; ++q)
            if (total[q] == 0) { fprintf(stderr, "never reached in any case: %s\n", reach_name[q]); ++bad; }
    printf("ahead: %d cases, %d failed\n", ran, bad);
    return bad ? 1 : 0;
}
#endif
