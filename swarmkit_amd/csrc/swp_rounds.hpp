// swp_rounds.hpp — every host rule of the block resolver's rounds, written once: the knobs, the row mode, runs and window, the block that
// fits the commit kernel's LDS, the pace (how many rounds to enqueue before the next look, and with which block), and what the single
// engine's driver adds to it: the compact switch, the hand-over to the scan resolver, and the two together as one stretch's rules
// (RoundRules). batch_run_impl (one engine) uses all of it, swp_shard_run (G engines in one process) and swp_shard_run_rank (one engine
// per rank) the knobs, the row mode, the fit and the pace; between ranks every rank MUST derive the same chunk and the same block from
// the same gathered words, or their collectives stop lining up. The drivers keep the mechanics (launches, read-backs, events, reports).
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
    int runs = -1;               // SWP_R6_RUNS: -1 unset (the batch decides: r6_shape), else 0 / 1 (tests, A/B runs)
    int compact = -1;            // SWP_R6_COMPACT: -1 unset (the rounds' symptom decides: CompactSwitch), 0 never, 1 from the first round on
    bool compact_fused = true;   // SWP_R6_COMPACT_FUSED=0: the index of the next round by a launch of its own, not at the end of k_r6_commit_c
    bool scan = true;            // SWP_SCAN=0: never hand a stretch to the scan resolver
    bool scan_compact = true;    // SWP_SCAN_COMPACT=0: nor, on a cluster beyond the scan resolver's node count, one whose class rows' union would fit (no probe)
    bool twins = true;           // SWP_R6_TWINS=0: every list starts at its level's first candidate
    int levels = -1;             // SWP_R6_LEVELS: -1 unset and 1: lists over two levels where the rule allows them (r6_levels2), 0: never
    int ring = -1;               // SWP_R6_RING: -1 unset (the rule decides: r6_ring), 0 never, 1 wherever the kernel allows it (tests, A/B runs)
};
inline int r6_knob01(const char* name) {   // -1 unset, else 0 / 1
    const char* env = getenv(name);
    return env ? (atoi(env) != 0 ? 1 : 0) : -1;
}
inline R6Knobs r6_knobs(uint32_t block_max, uint32_t default_cap) {
    R6Knobs k;
    const char* env_dbg = getenv("SWP_DBG");
    k.dbg = env_dbg ? (uint32_t)atoi(env_dbg) : 0u;
    const char* env_blk = getenv("SWP_R6_BLOCK");
    k.block_forced = env_blk != nullptr;
    k.block_cap = std::min<uint32_t>(block_max, std::max<uint32_t>(1u, env_blk ? (uint32_t)atoi(env_blk) : default_cap));
    k.task_rows = r6_knob01("SWP_R6_TASKROWS");
    k.runs = r6_knob01("SWP_R6_RUNS");
    k.compact = r6_knob01("SWP_R6_COMPACT");
    k.compact_fused = r6_knob01("SWP_R6_COMPACT_FUSED") != 0;
    k.scan = r6_knob01("SWP_SCAN") != 0;
    k.scan_compact = r6_knob01("SWP_SCAN_COMPACT") != 0;
    k.twins = r6_knob01("SWP_R6_TWINS") != 0;
    k.levels = r6_knob01("SWP_R6_LEVELS");
    k.ring = r6_knob01("SWP_R6_RING");
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

// A batch that is mostly RUNS of identical tasks (service-major order) keeps whole proposals in LDS and the blocks they allow: the
// runs-by-rank path (runs of >= 8) takes a run's picks from ONE task's window, and with windows of 16 in blocks of 1 408 service-major
// cfg3 — every task in a run of 100 — took 327 rounds and 12.6 ms where the parent took 288 and 10.2 (profiles/late_window.json,
// "major_windows_of_16"). Measured at the two ends only — no task in such a run (the headline), every task in one; the line between
// them is drawn at half the batch's tasks, counted once when the batch is built. SWP_R6_RUNS forces either; SWP_R6_BLOCK the block.
struct R6Shape { bool runs; uint32_t win, cap; };   // win: a proposal's entries in the commit kernel's LDS (0: late windows of 16); cap: tasks per round at most, before the fit
inline R6Shape r6_shape(const R6Knobs& k, uint32_t tasks_in_runs, uint32_t T) {
    const bool runs = k.runs >= 0 ? k.runs != 0 : 2u * (uint64_t)tasks_in_runs > T;
    return R6Shape{runs, runs ? 32u : 0u, (runs && !k.block_forced) ? std::min<uint32_t>(k.block_cap, 768u) : k.block_cap};
}

// Lists over two levels (swp_resolve6.hpp, R6Args.levels2): a complete list goes on with the task's candidates one level up that lie in
// front of it, so that the tasks which find their level used up where a lap over the node set ends are decided in the same round instead
// of cutting it (the headline: 126 rounds -> 73). It uses the room of the long lists, so it is on where they are (`ext_on`,
// RoundRules::ext(): not for a batch of runs, not for rounds whose block the pace has shrunk — the churn rounds, the compact index),
// and only on node sets with more half-words than a list holds (`list` = R6_LIST): on a smaller one a complete list names the whole
// level and what is in front of it is a handful of words. SWP_R6_LEVELS=0 switches it off; 1 is the default spelled out.
inline bool r6_levels2(const R6Knobs& k, bool ext_on, uint32_t n_words, uint32_t list) { return k.levels != 0 && ext_on && 2u * (uint64_t)n_words > list; }

// Ring rounds (swp_resolve6.hpp, R6Args.ring): the commit kernel keeps the windows and pick slots of fifteen 64-task groups, a slot per
// helper wave reused for each of its groups in turn, so a block is no longer what the LDS holds; what ends a longer block is the list,
// so a ring round's lists are R6_RING_LIST half-words long (a block of 2 816 picks is 88 half-words of one level's nodes). A round's
// fixed cost — two launches, the commit kernel's prologue and tail, two gaps — is paid per ROUND: the headline goes from 73 rounds of
// 1 408 to the model's 38 of 2 816 (tools/sim_window.py). On where ALL of these hold:
//   * the long lists are (`ext_on`, RoundRules::ext(): no batch of runs, no shrunk block — hence no churn rounds, no compact index);
//   * the batch has no cluster mounts (k_r6_commit_v has no ring) and the engine is single (the shard drivers never ask);
//   * the node set has more half-words than a ring list holds: a small one cannot supply a long block's picks from one level;
//   * the stretch has more tasks left than a flat block holds (`left` > `flat_block`): a ring round of fewer is a flat round with longer lists;
//   * SWP_R6_BLOCK is not set: a forced block stays flat where it fits, as every test that pins a round count expects.
// SWP_R6_RING=0: never. =1: wherever the kernel allows it (the first two lines), whatever the node set, the rest of the stretch and a
// forced block — which is then the ring block (r6_ring_block).
constexpr uint32_t R6_RING_TASKS = 960;     // = R6_RING: fifteen slots of 64 tasks
constexpr uint32_t R6_RING_LIST = 128;      // = R6_LIST_RING
constexpr uint32_t R6_RING_BLOCK = 2816;    // = R6_BMAX; 44 groups
inline bool r6_ring(const R6Knobs& k, bool ext_on, bool mounts, bool single, uint32_t n_words, uint32_t left, uint32_t flat_block) {
    if (k.ring == 0 || !ext_on || mounts || !single) return false;
    if (k.ring > 0) return true;
    return !k.block_forced && 2u * (uint64_t)n_words > R6_RING_LIST && left > flat_block;
}
// the block of a ring round: R6_RING_BLOCK, or what SWP_R6_BLOCK says (with SWP_R6_RING=1), in whole groups, within [64, ring_block_max]
inline uint32_t r6_ring_block(const R6Knobs& k, uint32_t asked, uint32_t ring_block_max) {
    const uint32_t b = k.block_forced ? asked : R6_RING_BLOCK;
    return std::min<uint32_t>(ring_block_max / 64u * 64u, std::max<uint32_t>(64u, b / 64u * 64u));
}
// The streamed driver publishes every `every` rounds of a flat block; ring rounds keep that cadence in TASKS
inline uint32_t r6_ring_stream_every(uint32_t every, uint32_t flat_block, uint32_t ring_block) {
    return (uint32_t)std::max<uint64_t>(1u, (uint64_t)every * flat_block / std::max<uint32_t>(ring_block, 1u));
}

// The words of the control block the rules below read after a chunk of rounds or behind a scan stretch, all running totals: decided up
// to pos; rounds that found work; rounds cut by an exhausted list or a window that ran out; rounds that had a compact index; matcher
// stops at an emptied half-word; tasks the batched scan answered without a look.
struct R6Words { uint32_t pos, rounds, cuts, crounds, reseats, scan_skipped; };

// The compact index (swp_resolve6.hpp, R6Args.compact): one more small launch per round, worth it when the level the tasks aim at is a
// sparse set of nodes (re-placements after a drain): the matcher then stops at an emptied half-word every few tasks and the rounds are
// cut by exhausted lists after a fraction of their block. Switched on by that symptom (a stop per <= 12 decided tasks; ordinary
// batches have one per 30-40), off again when the kernel found no such level in a whole chunk. `ever` (some chunk had rounds with an
// index) is the next batch's hint: a churn round's batch ENDS on tasks that aim at a level every node has, and a hint that said "the
// last chunk had one" began every batch with sixteen rounds without the index. (Starting with the previous batch's small BLOCK as well
// was measured and lost: device 3.39 -> 3.62 ms a round, same box, three runs each.)
struct CompactSwitch {
    bool ok, pinned, fused, on, ever = false;   // ok: may be built at all; pinned: SWP_R6_COMPACT non-zero, on whatever the rounds say
    uint32_t cuts_seen = 0, crounds_seen = 0, stops_seen = 0;
    // allowed: the caller's LDS and volume test; hint: the engine's, from the batch before
    CompactSwitch(bool allowed, const R6Knobs& k, bool hint) : ok(allowed && k.compact != 0), pinned(k.compact > 0), fused(k.compact_fused), on(ok && (pinned || hint)) {}
    uint32_t compact() const { return on ? (fused ? 2u : 1u) : 0u; }   // R6Args.compact of the next chunk
    // after a chunk: `used` rounds found work and decided `recent` tasks each, with blocks of `block`
    void feed(uint32_t used, double recent, uint32_t block, const R6Words& w) {
        const uint32_t exh = w.cuts - cuts_seen, cr = w.crounds - crounds_seen, stops = w.reseats - stops_seen;
        cuts_seen = w.cuts;
        crounds_seen = w.crounds;
        stops_seen = w.reseats;
        if (on && cr) ever = true;
        if (!ok || pinned) return;
        if (!on && used >= 4 && 2 * exh >= used && recent < 0.4 * block && (double)stops * 12.0 >= recent * used) on = true;
        else if (on && used >= 4 && cr == 0) on = false;
    }
};

// Rounds that decide only a handful of tasks each: the tasks there have no plain candidates (their services run on every node that
// could take them) and a round ends behind the first of them. The scan resolver decides such a stretch one task after the other
// (swp_scan.hpp); afterwards the bitmaps are rebuilt and the rounds are tried again. Its batched instance (k_scanb) decides ~4 tasks a
// barrier and answers an unplaceable task's twins without a look: where it can run (`fast`), a stretch goes to it after four poor
// rounds and two probing rounds follow it; the one-task-a-barrier instance (~1 us a task) has to be worth more: eight poor rounds,
// four probes. (Sixteen rounds of ~40 us between two stretches were a sixth of the dense batch.)
//
// CONDITIONAL (`probed`: a cluster of more nodes than the scan resolver takes): a stretch may go only if the union of its tasks' static
// class rows has at most `max_nodes` nodes (swp_scan.hpp, the compact instance). The driver probes [pos, upto) when due() says so — two
// small launches and one read-back — and asks fits(); too wide, it may try ONCE with shorter() (an eighth, at least 64 tasks: a
// service-major batch has one pool at a time, a round-robin batch over many pools does not); refused() otherwise, and the rounds carry on
// as they would have. A refused probe is not repeated at every look: the next one waits until the rounds have decided `hold` more tasks,
// and `hold` doubles with every refusal (2 048, 4 096, ...) and never shrinks. T tasks of rounds that can never be scanned so pay at
// most ceil(log2(T / 2048 + 1)) refusals of at most two probes each: 8 probes at T = 20 000, 18 at a million. While a refusal holds, the
// chunks are not shortened either (cap_chunk): the rounds look as often as they would without a scan resolver.
struct ScanHandover {
    bool ok, fast;
    bool probed = false;       // the hand-over is conditional (above); `fast` is off then: whether the batched instance takes a stretch is known behind its probe (looks)
    uint32_t max_nodes = 0;
    uint32_t hold = 2048, hold_until = 0;   // after a refusal: no probe before the rounds have reached task hold_until
    uint32_t probes = 0, refusals = 0;      // probes enqueued (the driver counts), stretches refused
    uint32_t len = 2048;       // tasks of the next stretch: still no plain candidates afterwards, and it is twice as long
    bool after_scan = false;   // the rounds since the last stretch: a few of them say whether the tasks still have no plain candidates
    uint32_t skipped_seen = 0, scanned = 0;
    ScanHandover(bool ok_, bool fast_) : ok(ok_), fast(ok_ && fast_) {}
    static ScanHandover conditional(bool ok_, uint32_t max_nodes_) {
        ScanHandover s(ok_, false);
        s.probed = true;
        s.max_nodes = max_nodes_;
        return s;
    }
    bool held(uint32_t pos) const { return probed && pos < hold_until; }
    bool due(uint32_t used, double recent, uint32_t left, uint32_t pos = 0xFFFFFFFFu) const {
        return ok && !held(pos) && used >= (fast ? (after_scan ? 2u : 4u) : (after_scan ? 4u : 8u)) && recent < 8.0 && left >= 64;
    }
    bool fits(uint32_t union_nodes) const { return union_nodes >= 1 && union_nodes <= max_nodes; }
    uint32_t shorter(uint32_t pos, uint32_t upto) const { return pos + std::max<uint32_t>(64u, (upto - pos) / 8u); }   // (due(): at least 64 tasks are left; never beyond upto)
    void refused(uint32_t pos) {
        ++refusals;
        hold_until = (uint32_t)std::min<uint64_t>(0xFFFFFFFFu, (uint64_t)pos + hold);
        hold = std::min<uint32_t>(hold * 2u, 1u << 30);
    }
    uint32_t upto(uint32_t pos, uint32_t end) const { return (uint32_t)std::min<uint64_t>(end, (uint64_t)pos + len); }
    uint32_t took(uint32_t pos, uint32_t upto) {   // the stretch [pos, upto) was enqueued -> the probing rounds behind it
        scanned += upto - pos;
        if (probed) len = std::max<uint32_t>(upto - pos, 64u);   // (where only a shorter stretch fitted, the next one is twice THAT long)
        len = std::min<uint32_t>(len * 2, 1u << 20);
        after_scan = true;
        return fast ? 2u : 4u;
    }
    // the words are read behind a node-local stretch of the batched instance: for `again`, and at the end for the driver's report only.
    // stretch_fast: a conditional hand-over's stretch that the batched instance took — fast is the
    // STRETCH's property then, not the rules'; the next stretch gets its own probe first (its union may differ).
    bool looks(bool node_local, uint32_t upto, uint32_t end, bool report, bool stretch_fast = false) const { return node_local && (fast || (probed && ok && stretch_fast)) && (upto < end || report); }
    // Most of the stretch was answered without a look (identical tasks had found no node — a saturated cluster's backlog): the kernel
    // does that at a hundred tasks a microsecond, a round of the block resolver at ten. Another stretch directly behind this one.
    bool again(uint32_t pos, uint32_t upto, uint32_t end, uint32_t scan_skipped) {
        const uint32_t sk = scan_skipped - skipped_seen;
        skipped_seen = scan_skipped;
        return upto < end && 2 * (uint64_t)sk >= upto - pos;
    }
    // look again soon: rounds that hit such a stretch decide one task each. Conditional: only rounds that ARE poor look sooner (sixteen
    // of them decide fewer than 256 tasks) — a batch that is doing well is left the chunks it would have without a scan resolver — and
    // none while a refusal holds.
    uint32_t cap_chunk(uint32_t chunk, double recent, uint32_t pos = 0xFFFFFFFFu) const {
        if (probed) return (ok && !held(pos) && recent < 16.0) ? std::min<uint32_t>(chunk, 16u) : chunk;
        return !ok ? chunk : std::min<uint32_t>(chunk, fast ? (recent < 16.0 ? 8u : recent < 64.0 ? 16u : 256u) : (recent < 16.0 ? 16u : recent < 64.0 ? 48u : 256u));
    }
};

// One stretch of the single engine's rounds: pace, switch and hand-over together. The driver enqueues pace.chunk rounds with pace.block,
// cpt.compact() and ext(), reads the words and asks after_rounds; where that says so it enqueues the scan stretch [pace.pos, scan_upto()),
// reads the words again where scan.looks says so, and asks after_scan — until pace.pos reaches pace.end.
struct RoundRules {
    RoundPace pace;
    CompactSwitch cpt;
    ScanHandover scan;
    bool ext_ok;   // lists beyond a proposal's 32 entries: not for a batch of runs, whose windows hold a whole proposal ...
    bool ext() const { return ext_ok && pace.block >= (flat ? flat : pace.largest); }   // ... nor for rounds whose block the pace has shrunk (below the largest FLAT block)
    // Ring rounds (r6_ring). A stretch that may have them is paced with the ring block as its largest (the driver builds `pace` so) and
    // carries the largest FLAT block here; 0: none in this stretch, block() is the pace's as ever. A round that is not a ring round —
    // the stretch's tail, a shrunk block, rounds with a compact index — lies in LDS as a whole: at most `flat` tasks. (Ring rounds that
    // decide less than 0.4 of their block make the pace shrink it; down to the flat block the rounds are what they are without a ring,
    // long lists included, and the pace grows the block again when they fill it.)
    uint32_t flat = 0;
    bool ring_mounts = false;
    uint32_t n_words = 0;
    R6Knobs ring_knobs{};
    bool ring() const { return flat != 0 && !cpt.on && pace.block >= pace.largest && r6_ring(ring_knobs, ext(), ring_mounts, true, n_words, pace.end - pace.pos, flat); }
    uint32_t block() const { return (flat == 0 || ring()) ? pace.block : std::min<uint32_t>(pace.block, flat); }
    // The words behind a chunk. true: a stretch goes to the scan resolver, and the rounds behind it keep block and ext (no replan);
    // false: the next chunk and the next block are planned. `used` is taken before the pace moves on.
    bool after_rounds(const R6Words& w, uint32_t* used, double* recent) {
        const uint32_t block = pace.block;
        *used = w.rounds - pace.rounds_seen;
        *recent = pace.observe(w.pos, w.rounds);
        cpt.feed(*used, *recent, block, w);
        if (scan.due(*used, *recent, pace.end - pace.pos, pace.pos)) return true;
        plan_rounds(*recent);
        return false;
    }
    void plan_rounds(double recent) {
        scan.after_scan = false;
        pace.replan(recent);
        pace.chunk = scan.cap_chunk(pace.chunk, recent, pace.pos);
    }
    // the probe found the stretch, and a shorter one, too wide: the rounds carry on as if after_rounds had said false
    void scan_refused(double recent) {
        scan.refused(pace.pos);
        plan_rounds(recent);
    }
    uint32_t scan_upto() const { return scan.upto(pace.pos, pace.end); }
    // The stretch [pace.pos, upto) was enqueued; `looked`: the words behind it, or null where scan.looks said no. true: another one.
    bool after_scan(uint32_t upto, const R6Words* looked) {
        pace.chunk = scan.took(pace.pos, upto);
        const bool again = looked && scan.again(pace.pos, upto, pace.end, looked->scan_skipped);
        pace.pos = upto;
        return again;
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

// One-off tasks with spread preferences inside a batch (swp_scan_spread.hpp): the SPREAD SEGMENTS of a range of tasks [j0, j1).
// kind(j): SPREAD_PLAIN — the task has no preferences and the spread kernel could take it as a tree of one leaf; SPREAD_TASK — it has
// preferences; SPREAD_FENCE — the spread kernel cannot take it (cluster mounts): it is never inside a segment.
// A segment STARTS at a task with preferences and ENDS in front of the first fence, or in front of the first run of at least
// SPREAD_GAP consecutive plain tasks, or at j1 — fewer plain tasks than that between two tasks with preferences, or behind the last
// one, ride along. Exactness does not depend on the rule (a plain task gets the same node from either resolver); hand-over cost does:
// a stretch of the block resolver behind a segment costs a rebuild of its bitmaps, its first rounds and a look at the control block
// — some 50 - 100 us, what the spread kernel needs for a few dozen tasks at its ~2 us each.
// on_seg(first, count, spread) for every piece of [j0, j1), in order, the pieces between segments included; returns the spread segments.
enum { SPREAD_PLAIN = 0, SPREAD_TASK = 1, SPREAD_FENCE = 2 };
constexpr uint32_t SPREAD_GAP = 64;
template <class K, class F>
inline uint32_t spread_segments(uint32_t j0, uint32_t j1, K kind, F on_seg) {
    uint32_t n_seg = 0, plain0 = j0;   // plain0: where the piece in front of the next segment starts
    for (uint32_t j = j0; j < j1;) {
        if (kind(j) != SPREAD_TASK) { ++j; continue; }
        uint32_t end = j + 1, gap = 0;   // end: one past the last task that is certainly inside; gap: plain tasks seen behind it
        for (uint32_t k = j + 1; k < j1; ++k) {
            const int c = kind(k);
            if (c == SPREAD_FENCE) break;
            if (c == SPREAD_TASK) { end = k + 1; gap = 0; continue; }
            if (++gap >= SPREAD_GAP) break;
            if (k + 1 == j1) end = j1;   // (a short tail rides along)
        }
        if (j > plain0) on_seg(plain0, j - plain0, false);
        on_seg(j, end - j, true);
        ++n_seg;
        plain0 = j = end;
    }
    if (j1 > plain0) on_seg(plain0, j1 - plain0, false);
    return n_seg;
}

}  // namespace swpdev
