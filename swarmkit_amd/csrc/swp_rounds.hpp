// swp_rounds.hpp — what the three drivers of the block resolver's rounds decide on the host, written once: the knobs, the row mode, the
// block that fits the commit kernel's LDS, and the pace (how many rounds to enqueue before the next look, and with which block).
// batch_run_impl (one engine), swp_shard_run (G engines in one process) and swp_shard_run_rank (one engine per rank) use it; between
// ranks every rank MUST derive the same chunk and the same block from the same gathered words, or their collectives stop lining up.
// No HIP and no engine types in here: tests/emu/emu_rounds.cpp compiles this header alone with g++ (tests/test_rounds_cpu.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

namespace swpdev {

// Test / debugging knobs of the block resolver. Read once per driver call, never cached across calls (the tests change them between runs).
struct R6Knobs {
    uint32_t dbg = 0;            // SWP_DBG: bit 16 switches the in-kernel section timers and the drivers' reports on, bit 32 one line per chunk
    bool block_forced = false;   // SWP_R6_BLOCK is set: the block stays what it says (as far as the LDS allows), whatever the pace
    uint32_t block_cap = 0;      // tasks per round at most: the knob or default_cap, within [1, block_max]
    int task_rows = -1;          // SWP_R6_TASKROWS: -1 unset, else 0 / 1
};
inline R6Knobs r6_knobs(uint32_t block_max, uint32_t default_cap) {
    R6Knobs k;
    const char* env_dbg = getenv("SWP_DBG");
    k.dbg = env_dbg ? (uint32_t)atoi(env_dbg) : 0u;
    const char* env_blk = getenv("SWP_R6_BLOCK");
    k.block_forced = env_blk != nullptr;
    k.block_cap = std::min<uint32_t>(block_max, std::max<uint32_t>(1u, env_blk ? (uint32_t)atoi(env_blk) : default_cap));
    const char* env_tr = getenv("SWP_R6_TASKROWS");
    if (env_tr) k.task_rows = atoi(env_tr) != 0 ? 1 : 0;
    return k;
}

// Demand-class rows patched by every commit while the batch has few distinct reservations; rows per task of the block, rebuilt every
// round from the exact residuals, when it has many (a commit would cross too many thresholds) — no limit then. Over a set of shards:
// task rows as soon as one of them wants them.
inline bool r6_task_rows(const R6Knobs& k, bool classes_ok, uint32_t n_classes) { return k.task_rows >= 0 ? k.task_rows != 0 : (!classes_ok || n_classes > 128u); }

// What a kernel's dynamic LDS may take. The commit kernel stages the block's lists next to the TK row: a very large node set gets a
// smaller block, in steps of 64 tasks down to 64. (A block that does not fit even then is the caller's refusal.)
constexpr size_t R6_LDS_BUDGET = 160 * 1024 - 512;
template <class F>
inline uint32_t r6_fit_block(uint32_t block, F lds_of_block) {
    while (block > 64 && (size_t)lds_of_block(block) > R6_LDS_BUDGET) block = (block - 1u) / 64u * 64u;
    return block;
}

// The block follows the pace: rounds that are cut after a few dozen tasks — re-placements that all aim at the few emptied nodes — need
// not propose and stage hundreds of lists each; rounds that fill their block get the next size up. `recent`: tasks decided per round
// in the last stretch. The buffers stay where the LARGEST block put them.
inline uint32_t r7_next_block(uint32_t cur, uint32_t largest, double recent) {
    if (recent > 0.4 * cur) return std::min<uint32_t>(largest, cur * 2u);
    return std::min<uint32_t>(largest, std::max<uint32_t>(128u, ((uint32_t)(2.0 * recent) + 63u) / 64u * 64u));
}

// Rounds are enqueued blindly, `chunk` at a time; after each chunk the driver learns the position and the number of rounds that found
// work, and the pace says how many rounds to enqueue next and with which block.
struct RoundPace {
    uint32_t pos, end;          // the stretch's tasks: decided up to pos, of [.., end)
    uint32_t rounds_seen = 0;
    uint32_t chunk;             // rounds to enqueue before the next look
    uint32_t block;             // tasks per round of the next chunk
    uint32_t largest;
    bool forced;
    RoundPace(uint32_t n_tasks, uint32_t largest_block, bool block_forced, uint32_t start = 0)
        : pos(start), end(start + n_tasks), chunk(std::min<uint32_t>(16u, (n_tasks + 255u) / 256u + 1u)),   // a short stretch does not pay for empty rounds
          block(largest_block), largest(largest_block), forced(block_forced) {}
    // the words read after a chunk -> tasks decided per round that found work
    double observe(uint32_t pos_now, uint32_t rounds_now) {
        const double recent = (double)(pos_now - pos) / (double)std::max<uint32_t>(rounds_now - rounds_seen, 1);
        rounds_seen = rounds_now;
        pos = pos_now;
        return recent;
    }
    // as many rounds as the rest needs at the pace so far, and a few more (a round past the end is a handful of empty launches); the next block
    void replan(double recent) {
        chunk = (uint32_t)std::min<double>(4096.0, (double)(end - pos) / std::max(1.0, recent) * 1.05 + 4.0);
        if (!forced && pos < end) {
            block = r7_next_block(block, largest, recent);
            if (block < largest) chunk = std::min<uint32_t>(chunk, 64u);   // (look again before long while the block is small)
        }
    }
    double advance(uint32_t pos_now, uint32_t rounds_now) {
        const double recent = observe(pos_now, rounds_now);
        replan(recent);
        return recent;
    }
};

// The streamed driver (swp_batch_run_streamed): behind every `every` rounds, every scan stretch and every k_waterfill run a publish
// (swp_publish.hpp) copies the decided prefix to host-visible memory and appends its end — a MARK — to a ring. This is what the host
// makes of the marks: which of them end a delivery to the caller's sink. Marks never go back; a publish that found no progress repeats
// the last one. A delivery holds at least max(min_tasks, 1) tasks, except the one that ends at T; with min_tasks = 0 every mark that
// moved is one delivery, so the sequence of calls is a function of the marks alone, never of when the host looked.
inline uint32_t stream_every() {   // SWP_STREAM_EVERY: rounds between two publishes (default 8)
    const char* env = getenv("SWP_STREAM_EVERY");
    const int v = env ? atoi(env) : 8;
    return (uint32_t)std::min(std::max(v, 1), 4096);
}
struct StreamMarks {
    static constexpr uint32_t RING = 4096;   // marks the ring holds: the driver drains it before that many are outstanding
    uint32_t T, min_tasks;
    uint32_t delivered = 0;   // [0, delivered) has gone to the sink
    uint32_t top = 0;         // the highest mark taken: [0, top) is final and in host memory
    uint32_t taken = 0;       // marks read off the ring
    uint32_t enqueued = 0;    // publishes enqueued (each appends exactly one mark)
    bool bad = false;         // a mark beyond T or behind an earlier one: the ring does not hold what the device wrote
    StreamMarks(uint32_t n_tasks, uint32_t min_tasks_) : T(n_tasks), min_tasks(min_tasks_) {}
    // one mark off the ring, in order; true: [*first, *first + *count) is due
    bool take(uint32_t mark, uint32_t* first, uint32_t* count) {
        ++taken;
        if (mark > T || mark < top) { bad = true; return false; }
        top = mark;
        const uint32_t pending = top - delivered;
        if (pending == 0 || (pending < min_tasks && top < T)) return false;
        *first = delivered;
        *count = pending;
        delivered = top;
        return true;
    }
    uint32_t outstanding() const { return enqueued - taken; }
    bool room() const { return outstanding() + 1u < RING; }        // another publish may be enqueued without a drain first
    bool complete() const { return !bad && delivered == T; }       // after the last mark: every task went out exactly once
};

// The streamed tick of task groups (swp_schedule_groups_streamed): ONE launch decides group after group, and the kernel itself appends
// the marks (swp_groups.hpp G2_OP_PUBLISH) — there is nothing between rounds where the host could drain the ring, and the kernel never
// waits for the host. So the rule is one the host can compute up front from the sizes alone: a mark behind group g iff the groups since
// the previous mark hold at least `step` tasks, or g is the last group. A tick never has more marks than groups; one of more than
// RING / 2 groups gets a step of at least total / (RING / 2), rounded up: a tick's marks then fill at most half the ring, whatever
// the knob says.
inline uint32_t stream_group_tasks() {   // SWP_STREAM_GROUP_TASKS: tasks between two marks of a streamed tick, at least (default 1024)
    const char* env = getenv("SWP_STREAM_GROUP_TASKS");
    const long long v = env ? atoll(env) : 1024;
    return (uint32_t)std::min<long long>(std::max<long long>(v, 1), 0x7FFFFFFF);
}
inline uint32_t group_pub_step(uint64_t total, uint32_t n_groups, uint32_t knob) {
    const uint64_t half = StreamMarks::RING / 2;
    const uint64_t floor_ = n_groups > half ? (total + half - 1) / half : 1;
    return (uint32_t)std::max<uint64_t>(std::max<uint32_t>(knob, 1u), floor_);
}
inline bool group_mark_due(uint32_t since, uint32_t step, bool last) { return since >= step || last; }   // (the kernel's test, word for word)
// on_mark(mark, group) for every mark of the tick, in order; returns how many there are
template <class F>
inline uint32_t group_marks(const uint32_t* sizes, uint32_t n_groups, uint32_t step, F on_mark) {
    uint32_t marks = 0, since = 0, end = 0;
    for (uint32_t g = 0; g < n_groups; ++g) {
        since += sizes[g];
        end += sizes[g];
        if (group_mark_due(since, step, g + 1 == n_groups)) {
            on_mark(end, g);
            since = 0;
            ++marks;
        }
    }
    return marks;
}

}  // namespace swpdev
