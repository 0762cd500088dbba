// swp_resolve6.hpp — the BLOCK resolver: the sequential argmin + commit pass of the tick (nodeSet.tree with a heap of one,
// nodeset.go:50-124; nodeLess, scheduler.go:708-735; NodeInfo.addTask, nodeinfo.go:108-154). The whole chip builds the candidate
// lists, one wave matches them. The engine's resolver for a one-off batch on a single engine, at every batch size.
//
// State in global memory (L2-resident), all of it bitmaps over the node words, kept exact by every commit:
//   planes[b]   bit b of (ActiveTasksCount − base) per node, base = the lowest count among the valid nodes at build time
//   rr[c]       ResourceFilter (filter.go:77-84) as set membership: nodes whose residual cpu (rows 0..n_dc−1) / memory (rows n_dc..)
//               is >= the row's threshold; thresholds = the batch's distinct reservations. In TASK-ROWS mode (a batch with more
//               than 128 of them) the rows are built per task of the coming block instead (k_r6_taskrows): no limit.
//   rg[r]       generic reservations (filter.go:86-91): nodes whose count of the row's kind is >= the row's value
//   sc, X, portmap   static class rows, per-service exception bitmaps, host ports: the rows every resolver uses
//
// One ROUND decides a block of up to `block` tasks, two launches:
//   k_r6_propose   one workgroup of eight wavefronts per task, lanes over the node WORDS: m = sc & ~X & RC & RM & RG & ~ports (the
//                  task's plain candidates, 64 nodes per operation); the level planes of a lane's words are requested together and
//                  the candidates are narrowed from the top plane down IN REGISTERS (m & ~plane ≠ ∅ ? keep that : the bit is set in
//                  the word's minimum level); one reduction gives the task's minimum level, the words whose own minimum equals it
//                  hold exactly its candidates. The first 2 * R6_CAND non-empty half-words go into the task's proposal, with the
//                  best node of the service's exception list by the full key when there is no plain candidate; up to R6_LIST in all
//                  with the side record R6Args.ext. A complete list goes on, where the host says so (R6Args.levels2), with a SECOND SECTION:
//                  the task's candidates one level up that lie in front of the first section ("the second section" in r6_propose_t).
//   k_r6_commit    one workgroup of 1 024. LDS holds a window of every task's list (entry-major): its first R6_WIN entries that are live
//                  when its group is staged — groups 0 and 1 by the prologue, group g by its applying wave two groups ahead of the
//                  matcher (r6_commit_t). Wave 0 walks the block in task order, 64 tasks at a time: a lane seats the first two half-words of its list that still have a candidate
//                  (cursor: an entry is looked at once) and wv::match_seq64 gives every task in turn the first listed node nobody
//                  before it took, struck from every later list. The block is CUT — committed up to there, proposed again from
//                  there — in front of a task whose listed nodes are all taken, around a task that must use its exception list
//                  (its order moves with every placement of the service) and behind an uncounted task (its node did NOT move
//                  up). Waves 1..15 (each takes every fifteenth group) move the cursors of "their" group over dead entries while they wait, then apply the group's
//                  picks: NodeInfo.addTask on the node rows + the bitmaps above + commit log.
//   k_r6_compact   (only while the host sees the symptom: a matcher stop every few tasks, rounds cut after a fraction of their block)
//                  one workgroup, in front of the round's propose: numbers the ready nodes on the level the block's first task aims
//                  at in node order. Tasks whose minimum level is that one list half-words of those POSITIONS — 32 candidates each
//                  where plain half-words hold three of the few emptied nodes — the others plain half-words behind them
//                  (R6Args.compact, the _c instances of the two kernels).
// The exactness argument is the list rule: inside a batch levels only grow and feasibility only shrinks, and a list
// holds ALL plain candidates of the task's minimum level in node order up to its last half-word. Half-words ascend PER SECTION: a list
// is in preference order, and the commit kernel takes its entries as opaque (half-word, bits) pairs in that order — the window staging,
// the cursor loops, the seating step, the runs-by-rank path and wv::match_seq64 compare half-words for equality only, never for order.
//
// Written against swp_wave.hpp only, so tests/emu runs the same source on CPU fibers (tests/test_emu_resolve6.py).
#pragma once
#include <stddef.h>

#include <type_traits>

#include "swp_shard.hpp"
#include "swp_types.hpp"
#include "swp_volumes.hpp"

namespace swpdev {

#define R6_NP 16                 // level planes: 65 535 levels above the lowest valid node
#ifndef R6_CAND
#define R6_CAND 16               // a proposal lists 2 * R6_CAND non-empty 32-node half-words: a block is cut where a task finds all its listed nodes taken
#endif
#define R6_SEAT 2                 // list entries a seating step of the matcher looks at (4 measured no better: fewer steps, each longer)
#ifndef R6_SEAT_AHEAD
#define R6_SEAT_AHEAD 1          // the matcher requests the entries at a lane's cursor when the cursor moves, not when it stops there (0: at the stop — A/B builds, tests/emu)
#endif
#ifndef R6_LEVELS2
#define R6_LEVELS2 1             // the propose kernels know the second list section (R6Args.levels2); 0: compiled out (A/B builds, tests/emu)
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define R6_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)   // the instruction scheduler moves nothing across this point (not a memory fence, no instruction)
#else
#define R6_SCHED_FENCE() ((void)0)
#endif
#ifndef R6_REACH
#define R6_REACH(what, cond)     // tests/emu counts the paths of the matcher a run came across (a driver defines it in front of this header); nothing in the product
#endif
#ifndef R6_RING_ON
#define R6_RING_ON 1             // the ring instance of the commit kernel and the long lists of its rounds (R6Args.ring); 0: compiled out (A/B builds — launch_r6_rounds
                                 // then refuses R6Args.ring, so run them with SWP_R6_RING=0 — and tests/emu)
#endif
#ifndef R6_RING_REACH
#define R6_RING_REACH(what, cond)   // tests/emu/emu_resolve6_ring.cpp counts the ring's own paths (R6RR_*); nothing in the product, nothing in the other drivers
#endif
#define R6_BMAX 2816             // largest block of a single engine (waves 1..15 of the commit kernel apply its 64-task groups in turn): a RING block
                                 // (R6Args.ring, the _r instances of the kernels); a flat block, which lies in LDS as a whole, ends at R6_FLAT_BMAX
#define R6_FLAT_BMAX 2048
#define R6_RING 960              // tasks of the commit kernel's ring: one slot of 64 tasks for each of its fifteen helper waves
#define R7_BMAX 1024             // ... of the node-range shards: one group per wave of their commit kernel
#define R6_COMMIT_THREADS 1024
#define R6_LIST 64               // half-words the propose kernels list at most: the first 2 * R6_CAND in the proposal, the others in its extension (R6PropExt)
#define R6_LIST_RING 128         // ... in a ring round (R6Args.ring): a block of 2 816 picks is 88 half-words of one level's nodes
#ifndef R6_WIN
#define R6_WIN 16                // list entries of a task the commit kernel keeps in LDS: the first that are live when the task's group is staged
#endif
#define R6_NONE 0xFFFFFFFFu

enum { R6RR_SKIPPED3, R6RR_WRAPPED_STAGE, R6RR_N };   // R6_RING_REACH: a staging that skipped >= 3 dead batches of sixteen; a stage() into a reused slot
struct Blk6 {   // control block, global memory
    u32 pos, end;          // next undecided task, end of the stretch
    u32 base, maxrel;      // lowest task count among the valid nodes at build time; highest level above it so far
    u32 error, rounds, cut_exhausted, cut_exception, cut_uncounted;
    u32 cyc[4];            // R6Args.dbg & 16: shader cycles / 64 of k_r6_commit's sections (prologue, matching, wait for it, apply)
    u32 reseats, cyc_load, cyc_walk;   // how often the matcher stopped at an emptied half-word (always counted); dbg: cycles / 64 of a group's list load and of its walk
    u32 cyc_g[4];          // ... of the list load: waiting for the group's lists, the head records, seating; seating steps
    u32 csize, clevel;     // compact index of this round (k_r6_compact): its nodes (0: none, every list in plain half-words), their level above the base
    u32 crounds;           // rounds that had one
    u32 dbg_cut[3];        // dbg: of the cuts at an exhausted list, those whose list was full (more candidates on the level), in compact positions, one entry long
    u32 scan_skipped;      // k_scanb: tasks answered "no node" without a look (an identical task found none earlier in the stretch)
    u32 scan_batches;      // k_scanb: barriers it took for the tasks it did look at
    u32 cut_window;        // cuts in front of a task whose LDS window ran out while something lay behind it: live entries, entries nobody looked at
                           // (possibly dead), or more of the level than was listed (bit 31) — an upper bound of the cuts a whole list would have avoided; not in cut_exhausted
    u32 cyc_h[3];          // dbg: cyc_g[1] split — up to the first use of the head record / template id, the flags and the cursor from LDS, the run path
    u32 dbg_late_runs;     // dbg: tasks whose pick the runs-by-rank path took in a group >= 2 (descriptor ids a helper left in the group's pick slots)
    u32 cyc_s[3];          // dbg: cyc_walk split (and what follows it) — inside wv::match_seq64, the stops (a walk's return to the next walk's entry, or to
                           // the cut at an exhausted list), a group's epilogue (its last walk's end to the publish of its picks)
    u32 dbg_walks;         // dbg: calls of wv::match_seq64
    u32 dbg_lv2;           // dbg: proposals that carried a second section (R6Args.levels2), counted by the propose kernel
};
static_assert(sizeof(Blk6) == 152, "Blk6 layout");

struct R6Prop {   // one task's proposal: the shard protocol's record (include/swp.h swp_proposal) with more candidates, as 32-node half-words
    u32 level, n_cand;       // minimum level among the plain candidates (R6_NONE: there is none); half-words listed | bit 31: there are more
                             // (R6Args.levels2: the entries of a second section count; `level` stays the first section's; bit 31: the room cut the second)
    unsigned short hw[2 * R6_CAND];   // half-word index (node = 32 * hw + bit), ascending PER SECTION (the list is in preference order: the level's half-words, then —
                                      // R6Args.levels2 — half-words of the next level that all lie in front of them): the first 2 * R6_CAND NON-EMPTY half-words — 16 bits
                                      // (round 6: node sets end at 2^21 nodes): a record is 224 bytes instead of 288, to write, to stage, to fold and to all-gather
    u32 hb[2 * R6_CAND];     // the level's survivors inside each
    u64 exc_hi, exc_lo;      // best node of the service's exception list by nodeLess' key, KEY_NONE: none
    u32 exc_entry, flags;    // flags bit 0: the task does not count on its node; bit 1: it has cluster mounts
};
static_assert(sizeof(R6Prop) == 8 + 12 * R6_CAND + 24, "R6Prop layout");
static_assert(2 * R6_CAND <= 64, "one lane per list entry");
struct R6PropExt {   // entries 2 * R6_CAND .. R6_LIST - 1 of a task's list (R6Args.ext): read by the commit kernel only, never sent between shards
    unsigned short hw[R6_LIST - 2 * R6_CAND];
    u32 hb[R6_LIST - 2 * R6_CAND];
};
struct R6PropExtRing {   // ... of a RING round (R6Args.ring), entries up to R6_LIST_RING - 1: what R6Args.ext points to there, for the _r instances alone —
                         // a flat round's records, and the flat instances' code, are what they were without a ring
    unsigned short hw[R6_LIST_RING - 2 * R6_CAND];
    u32 hb[R6_LIST_RING - 2 * R6_CAND];
};
static_assert(R6_WIN >= 1 && R6_WIN <= 2 * R6_CAND && R6_LIST % 16 == 0 && R6_LIST_RING % 16 == 0 && (2 * R6_CAND) % 16 == 0, "the window staging reads 16 entries a batch");
static_assert(R6_LIST <= R6_LIST_RING && R6_RING == 15 * 64 && R6_BMAX % 64 == 0 && R6_FLAT_BMAX <= R6_BMAX, "ring geometry");

struct R6Args {
    u32 n_nodes, n_words, xs, block;
    u32 n_dc, n_dm;
    u32 dbg;                 // timing experiments only (env SWP_DBG); 0 in production
    u32 task_rows;           // != 0: ResourceFilter rows per TASK of the block, rebuilt every round (k_r6_taskrows), instead of per demand class
    const u64* valid;        // [n_words]
    const u64* sc;           // [n_sc][n_words]
    u64* X;                  // [n_svc][xs]
    const RTask* rt;
    i64* cpu;
    i64* mem;
    u32* total;
    u32* list_node;
    u32* list_svc;
    u32* list_fail;
    const u32* list_off;
    u64* portmap;
    const u32* pset_off;
    const u32* pset_ids;
    int32_t* out_node;
    u32* log_node;
    u32* log_task;
    int32_t* log_prev;
    int32_t* last;
    u32* inf_task;
    u32* inf_pos;
    Ctl* ctl;
    u64* planes;             // [R6_NP][n_words]
    u64* rr;                 // [n_dc + n_dm][n_words]
    const i64* thr;          // [n_dc + n_dm] the distinct cpu reservations (ascending), then the memory ones
    Blk6* blk;
    R6Prop* prop;            // [block]
    u64* trows;              // [block][n_words] task_rows mode: {cpu residual >= the task's NanoCPUs && memory residual >= its MemoryBytes}
    // generic reservations (filter.go:86-91, validate.go:24-52): n_rg more demand-class rows, rg[r] = {count[rg_kind[r]] >= rg_val[r]},
    // sorted by (kind, value); a task's set (tg[task] -> gs_off / gs_row) names its rows. n_rg == 0: none of the pointers is read.
    u32 n_rg, gstride;       // rows; node stride of gcnt
    int32_t* gcnt;           // [kind][gstride] the node's count of the kind (0: the kind is absent)
    u64* rg;                 // [n_rg][n_words]
    const u32* tg;           // [tasks of the batch] batch-local generic set, 0 = none
    const u32* gs_off;       // [sets + 1]
    const u32* gs_row;
    const u32* rg_kind;      // [n_rg]
    const int32_t* rg_val;   // [n_rg]
    const u32* rg_k0;        // [n_rg] first row of the row's kind ...
    const u32* rg_k1;        // ... and one past its last
    // [tasks of the batch] the first task of the batch with this task's descriptor: equal values = identical tasks, whose plain candidates
    // of a round are the same set. nullptr: lists start at the level's first candidate (the shard drivers: a range sees only its own part).
    const u32* tmpl;
    // CSI volumes (swp_volumes.hpp). csi_of == nullptr: the batch has no task with cluster mounts. Such a task's candidates depend on the
    // volumes every earlier one took — on ANY node — so a block decides at most one of them: the second one is where the block is cut.
    const u32* csi_of;       // [tasks of the batch] index among the batch's tasks with mounts, R6_NONE: it has none
    const u32* csi_set;      // [those tasks] mount set
    u64* vrows;              // [those tasks][n_words] VolumesFilter.Check (filter.go:424-432) as the volumes stood at the start of the task's last round
    u32* att;                // [those tasks][VOL_MAX_MOUNTS] the volumes chosen for its mounts on its node (chooseTaskVolumes), VOL_NONE: none
    VolView vol;
    // The compact index (k_r6_compact, one launch in front of a round's propose). Re-placements after a drain all aim at the few emptied
    // nodes: their level holds, say, 1 000 of 10 000 nodes, three to a half-word, so a list of 32 half-words names 100 of them and the
    // matcher's two seats hold six. The ready nodes ON the level the block's first task aims at, numbered in node order, are the round's
    // compact positions; a task whose minimum level is that one lists half-words of POSITIONS (dense: 32 candidates each), every other task plain half-words behind
    // them (+ 2 * ceil(csize / 64)). One level per list, so a list lives in one of the two address ranges; a node has one address per round,
    // so strikes meet; numbering in node order keeps every list in node order. The applying threads translate a picked address back.
    u32 compact;             // != 0: the rounds launch k_r6_compact and the kernels honour Blk6.csize; 2: k_r6_commit_c builds the NEXT round's index itself
                             // at its end (launch_r6_rounds: one k_r6_compact in front of a chunk's first round only)
    const u64* cbase;        // [n_words] the nodes an index is drawn from: READY && valid — every static class row is a subset, so every task's
                             // candidates are (a drained node keeps its place in `valid` and its level, which is usually the lowest)
    u64* cmask;              // [n_words] the nodes of the compact index
    u32* crank;              // [n_words] compact position of the word's first such node
    u32* cidx;               // [r6_compact_cap(n_words)] node of a compact position
    // node-range shards (swp_resolve7.hpp): where this shard publishes the volumes of a task with cluster mounts it placed ([2] slots, by
    // round parity, right behind its proposals — they travel with them); nullptr: no volumes in the batch
    struct R7Trail* trail_out;   // = the slots of its R7Tail
    // [block] the list entries beyond the proposal's; nullptr: lists end with the proposal (the shard drivers: the record they exchange)
    // (a ring round, `ring` below: [block] R6PropExtRing behind this pointer)
    R6PropExt* ext;
    u32 win;                 // list entries a task in the commit kernel's LDS (r6_win_of: 0 = R6_WIN); the launch sizes the LDS by it
    u32 no_runs;             // != 0: the batch has no run of >= 8 consecutive identical tasks (counted when it is built): the matcher leaves the
                             // runs-by-rank path and the descriptor ids it reads alone (its entry found nothing in every group of the headline:
                             // 4 650 of a round's 160 k cycles)
    u32 levels2;             // != 0: a complete list goes on with a SECOND SECTION, the task's candidates one level up that lie in front of the first
                             // section (r6_propose_t, "the second section"); 0: lists of one level. Honoured by the instances without a compact index
    u32 ring;                // != 0: a RING round (k_r6_commit_r; the host's rule: swp_rounds.hpp r6_ring). The commit kernel keeps the pick slots and the
                             // windows of `ring` tasks (R6_RING) instead of the block's: group g lives in slot g % 15, the slot of the helper that
                             // stages and applies it, so `block` may exceed what LDS holds; the propose kernels list up to R6_LIST_RING half-words.
                             // 0: the whole block in LDS, lists of R6_LIST
};
struct R7Args;   // swp_resolve7.hpp: what a shard's commit kernel knows of the other shards
#define R7_FOLDS_IN_FLIGHT 4u   // waves that fold at the same time (the R7 staging below); SWP_DBG bits 8-11 override it for A/B runs (tools/gpu_r5_foldwin.sh)
#define R7M_EXC 0x100u   // H_meta of a folded record: list length | the task has an exception-list candidate on some shard | it does not count on its node | it has cluster mounts
#define R7M_UNC 0x200u
#define R7M_CSI 0x400u
// A task's L_cur word in the single engine's commit kernel (not R7): cursor | entries in the window << 8 | the bits below. The wave that
// stages the task's window holds its record: it leaves what the matcher needs of the record's head here, so that wave 0 reads a group's
// set-up from LDS only. Every writer of the word carries them (the prologue, a helper's stage() and its cursor loop).
#define R6C_LEFT 0x10000u     // something of the list was left out of the window
#define R6C_PLAIN 0x20000u    // level != R6_NONE: the task has plain candidates
#define R6C_EXC 0x40000u      // exc_hi != KEY_NONE: its service's exception list has a candidate
#define R6C_UNC 0x80000u      // flags bit 0: it does not count on its node
#define R6C_CSI 0x100000u     // flags bit 1: it has cluster mounts
inline __host__ __device__ u32 r6_head_bits(u32 level, u64 exc_hi, u32 flags) {
    return (level != R6_NONE ? R6C_PLAIN : 0u) | (exc_hi != KEY_NONE ? R6C_EXC : 0u) | ((flags & 1u) ? R6C_UNC : 0u) | ((flags & 2u) ? R6C_CSI : 0u);
}

#define R6_UNROLL 4              // 64-word chunks a propose wave has in flight together ...
#define R6_SMALL_WORDS 512u      // ... on node sets beyond this many words (32 768 nodes); up to there a wave has ONE chunk: a quarter of the registers, so that
                                 // the workgroups of a large block are all resident at once
#define R6_PW 8                  // waves per task in the propose kernel
#define R6_PW_TINY 4u            // ... of its instance for node sets of up to R6_TINY_WORDS words (16 384 nodes): a chunk per wave
#define R6_TINY_WORDS 256u
inline __host__ __device__ u32 r6_unroll(u32 n_words) { return n_words <= R6_SMALL_WORDS ? 1u : (u32)R6_UNROLL; }
inline __host__ __device__ u32 r6_chunks(u32 n_words) { const u32 g = r6_unroll(n_words) * R6_PW; return (((n_words + 63u) >> 6) + g - 1u) / g * g; }
inline __host__ __device__ size_t r6_propose_lds(u32 n_words) { return (size_t)2 * r6_chunks(n_words) * 64 * 8 + 128; }
// TK row, thresholds, the picks of the block, a few scalars, the block's list windows (entry-major)
// (per task: pick node / index / aux, the cursor, R6_WIN candidate masks and as many half-word indices of 16 bits: node sets of up to 2^21 nodes)
// (the TK row: the node words, and in front of them the words of a compact index — at most a quarter of the nodes)
#define R6_COMPACT_MAX_WORDS 16384u   // node words up to which a compact index may be built (half-word indices are 16 bits in the commit kernel's LDS); the
                                      // engine sizes the block of such a node set so that the index's quarter more of TK row fits next to the windows (r6_cpt_room)
inline __host__ __device__ u32 r6_compact_cap(u32 n_words) { return 16u * n_words; }
inline __host__ __device__ u32 r6_tk_words(u32 n_words) { return n_words + n_words / 4u + 2u; }   // (with a compact index; n_words otherwise)
inline __host__ __device__ u32 r6_win_of(u32 win) { return win == 0 ? (u32)R6_WIN : win < 2u * R6_CAND ? win : 2u * R6_CAND; }
inline __host__ __device__ size_t r6_commit_lds(u32 n_words, u32 block, u32 n_rr, bool compact = false, u32 win = 0) {
    return (size_t)((compact ? r6_tk_words(n_words) : n_words) + n_rr) * 8 + (size_t)block * (16 + r6_win_of(win) * 6) + 192;
}
// ... of the ring instance (R6Args.ring): the TK row still covers the block (it is per node), picks and windows are the ring's, and
// staged[] is one flag per group of the BLOCK — the flat header's 32 flags are not enough — behind the 16 scalars
inline __host__ __device__ u32 r6_ring_flags(u32 block) { return ((block + 63u) / 64u + 15u) / 16u * 16u; }
inline __host__ __device__ size_t r6_commit_lds_ring(u32 n_words, u32 block, u32 n_rr, u32 ring, u32 win = 0) {
    return (size_t)(n_words + n_rr) * 8 + (size_t)ring * (16 + r6_win_of(win) * 6) + 64 + (size_t)r6_ring_flags(block) * 4;
}

#ifdef SWP_R6_KERNELS   // the kernels: swp_resolve6.hip and the emulation harness only (the engine TU shares the argument records)
// the node-range shards' side of the commit kernel (defined in swp_resolve7.hpp; only its R7 instances use them)
WV_DEV u32 r7_tk_words(const R7Args* m);
WV_DEV bool r7_any_dead(const R7Args* m);
WV_DEV void r7_fold_into(const R7Args* m, u32 i, bool have, u32 block, unsigned short* L_hw, u32* L_hb, u32* H_level, u32* H_meta, u32* sh);
WV_DEV u32 r7_addr(const R7Args* m, u32 shard, u32 node);
WV_DEV u32 r7_local(const R7Args* m, u32 addr, u32 my, bool* here);
WV_DEV u32 r7_take_trailers(const R6Args& a, const R7Args* m, u32 my, u32 round);
WV_DEV void r7_leave_trailer(const R6Args& a, u32 my, u32 round, u32 set, u32 node, const u32* att, u32 n);

// a counter many workgroups add to (reports under R6Args.dbg only). On the CPU fibers one thread runs at a time: a plain add.
#if defined(__HIPCC__)
WV_DEV void r6_count32(u32* p) { __hip_atomic_fetch_add(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#else
inline void r6_count32(u32* p) { *p += 1u; }
#endif

WV_DEV u64 r6_wave_min64(u64 v) {
    const u32 hi = (u32)(v >> 32), lo = (u32)v;
    const u32 mh = wv::min_u32(hi);
    const u32 ml = wv::min_u32(hi == mh ? lo : 0xFFFFFFFFu);
    return ((u64)mh << 32) | ml;
}

// ---- build: base / highest level (one workgroup of 1024), then planes and demand-class rows (one wave per node word) ----
WV_KERNEL(1024) void k_r6_minmax(R6Args a) {
    u32* red = reinterpret_cast<u32*>(wv::lds());
    u32 lo = 0xFFFFFFFFu, hi = 0;
    for (u32 n = wv::tid(); n < a.n_nodes; n += 1024)
        if ((a.valid[n >> 6] >> (n & 63)) & 1) {
            const u32 t = a.total[n];
            lo = min(lo, t);
            hi = max(hi, t);
        }
    lo = wv::min_u32(lo);
    hi = ~wv::min_u32(~hi);
    if (wv::lane() == 0) {
        red[wv::wave()] = lo;
        red[16 + wv::wave()] = hi;
    }
    wv::barrier();
    if (wv::tid() == 0) {
        for (u32 i = 1; i < 16; ++i) {
            lo = min(lo, red[i]);
            hi = max(hi, red[16 + i]);
        }
        if (lo == 0xFFFFFFFFu) lo = hi = 0;   // no valid node
        a.blk->base = lo;
        a.blk->maxrel = hi - lo;
        a.blk->error = (hi - lo) >> R6_NP ? (u32)ERR_LEVEL_RANGE : (u32)ERR_NONE;
    }
}

WV_KERNEL(256) void k_r6_rows(R6Args a) {
    const u32 w = wv::block() * 4 + wv::wave(), lane = wv::lane();
    if (w >= a.n_words) return;
    const u32 base = wv::uload(&a.blk->base);   // written by the launch before this one
    const u32 n = w * 64 + lane;
    const bool in = n < a.n_nodes;
    const bool v = in && ((wv::uload(a.valid + w) >> lane) & 1);
    const u32 lvl = v ? a.total[n] - base : 0u;
    for (u32 b = 0; b < R6_NP; ++b) {
        const u64 word = wv::ballot(v && ((lvl >> b) & 1u));
        if (lane == 0) a.planes[(size_t)b * a.n_words + w] = word;
    }
    const i64 qc = in ? a.cpu[n] : 0, qm = in ? a.mem[n] : 0;
    for (u32 c = 0; c < a.n_dc + a.n_dm; ++c) {
        const u64 word = wv::ballot(in && (c < a.n_dc ? qc : qm) >= wv::uload(a.thr + c));
        if (lane == 0) a.rr[(size_t)c * a.n_words + w] = word;
    }
    for (u32 r = 0; r < a.n_rg; ++r) {
        const u64 word = wv::ballot(in && a.gcnt[(size_t)wv::uload(a.rg_kind + r) * a.gstride + n] >= wv::uload(a.rg_val + r));
        if (lane == 0) a.rg[(size_t)r * a.n_words + w] = word;
    }
}

// ---- task rows: ResourceFilter.Check (filter.go:77-84) of every task of the coming block against the residuals as they are ------
// A batch whose tasks carry hundreds of distinct reservations (every service its own NanoCPUs / MemoryBytes) would make every commit
// cross hundreds of demand-class thresholds. For such a batch the rows are not kept per class and patched by the commits but built
// per task at the start of every round, from the exact residuals: one wave per node word (a ballot IS a row word), the block's
// reservations staged in LDS. No limit on the number of distinct reservations.
// `g_first`, `g_step`: the 64-task groups of the block this workgroup works for (k_r6_taskrows: one group per workgroup row of the
// grid, so that the launch fills the chip; the shard driver's launch uses its second grid dimension for the shards and walks all groups).
WV_DEV void r6_taskrows(const R6Args& a, u32 g_first, u32 g_step) {
    const u32 pos = wv::uload(&a.blk->pos), end = wv::uload(&a.blk->end);
    if (pos >= end || wv::uload(&a.blk->error) != ERR_NONE) return;
    const u32 cnt = min(a.block, end - pos);
    if (g_first * 64u >= cnt) return;
    i64* res = reinterpret_cast<i64*>(wv::lds());   // [block][2], a task without the filter: (INT64_MIN, INT64_MIN): every node passes
    for (u32 g0 = g_first * 64u; g0 < cnt; g0 += g_step * 64u)
        for (u32 j = g0 + wv::tid(); j < min(g0 + 64u, cnt); j += 256) {
            const RTask* rt = a.rt + pos + j;
            const bool on = (rt->flags & RT_RES) != 0;
            res[2 * j] = on ? rt->cpu : (i64)0x8000000000000000ull;
            res[2 * j + 1] = on ? rt->mem : (i64)0x8000000000000000ull;
        }
    wv::barrier();
    const u32 w = wv::block() * 4 + wv::wave(), lane = wv::lane();
    if (w >= a.n_words) return;
    const u32 n = w * 64 + lane;
    const bool in = n < a.n_nodes;
    const i64 qc = in ? a.cpu[n] : 0, qm = in ? a.mem[n] : 0;
    const u64 inmask = wv::ballot(in);
    // lanes = 64 tasks of the block at a time, the word's 64 residual pairs walked on the scalar side: ten instructions per (node, 64
    // tasks) and one store per lane and group, instead of a ballot and a one-lane store per task
    for (u32 g0 = g_first * 64u; g0 < cnt; g0 += g_step * 64u) {
        const u32 j = g0 + lane;
        const bool have = j < cnt;
        const i64 rc = have ? res[2 * j] : 0, rm = have ? res[2 * j + 1] : 0;
        u32 lo = 0, hi = 0;
        for (u32 i = 0; i < 32; ++i) {
            const i64 c0 = (i64)wv::readlane64((u64)qc, i), m0 = (i64)wv::readlane64((u64)qm, i);
            const i64 c1 = (i64)wv::readlane64((u64)qc, i + 32), m1 = (i64)wv::readlane64((u64)qm, i + 32);
            if (rc <= c0 && rm <= m0) lo |= 1u << i;
            if (rc <= c1 && rm <= m1) hi |= 1u << i;
        }
        if (have) a.trows[(size_t)j * a.n_words + w] = (((u64)hi << 32) | lo) & inmask;
    }
}

WV_KERNEL(256) void k_r6_taskrows(R6Args a) { r6_taskrows(a, wv::block_y(), (a.block + 63u) / 64u); }   // grid (words / 4, groups of the block)

// ---- volume rows: VolumesFilter.Check of the block's tasks with cluster mounts, from the volumes as they are (grid: words / 256, block) ----
WV_KERNEL(256) void k_r6_volrows(R6Args a) {
    const u32 pos = wv::uload(&a.blk->pos), end = wv::uload(&a.blk->end);
    const u32 t = pos + wv::block_y();
    if (t >= end || wv::uload(&a.blk->error) != ERR_NONE) return;
    const u32 ck = wv::uload(a.csi_of + t);
    if (ck == R6_NONE) return;
    const u32 w = wv::block() * 256 + wv::tid();
    if (w < a.n_words) a.vrows[(size_t)ck * a.n_words + w] = vol_filter_word(a.vol, wv::uload(a.csi_set + ck), w);
}

// ---- compact index: the ready nodes on the level the block's first task aims at, numbered in node order (one workgroup of 1 024) ----
// The level is the minimum among the plain candidates of the task at Blk6.pos (the rows the propose kernel combines, narrowed over the
// level planes the same way): after a drain that is the level of the emptied nodes, which the tasks behind it aim at as well — not the
// lowest level among the ready nodes, where nodes that nobody can use (no room, the wrong platform) sit for ever. The index holds ALL
// ready nodes on that level (their running count is a word's first position, crank; the nodes themselves go to cidx). More than a
// quarter of the node set on it, or no plain candidate: no index this round.
// (FUSED: the same pass at the END of k_r6_commit_c, for the round that follows — R6Args.compact == 2: the launch, its ramp and its drain
// are a fifth of a churn round. The rows it reads were changed by this workgroup's atomics a moment ago, so every load of a row that
// moves goes past the vector L1 (g_fresh*), and Blk6.maxrel — which the kernel's scalar loads may have cached with the control block —
// is read the same way. `t`: the first task of the coming round; `red`: 32 words of LDS nobody else uses any more.)
template <bool FUSED> WV_DEV void r6_compact_body(const R6Args& a, u32 t, u32* red) {
    const u32 tid = wv::tid(), lane = wv::lane(), wave = wv::wave();
    const u32 Wn = a.n_words;
    auto ld = [](const u64* q) { return FUSED ? wv::g_fresh64(q) : *q; };
    const u32 maxrel_v = FUSED ? wv::g_fresh32(&a.blk->maxrel) : 0u;   // (requested with the task's record, not in front of it)
    const RTask* rt = a.rt + t;
    const u32 flags = wv::uload(&rt->flags), svc = wv::uload(&rt->svc), scid = wv::uload(&rt->sc), pset = wv::uload(&rt->pset);
    const int nb = 32 - wv::clz32(FUSED ? wv::readfirstlane(maxrel_v) : wv::uload(&a.blk->maxrel));
    const u64* scrow = a.sc + (size_t)scid * Wn;
    const u64* xrow = a.X + (size_t)svc * a.xs;
    const bool res = (flags & RT_RES) != 0;
    const u64* rc = a.task_rows ? a.trows : a.rr + (size_t)((flags >> RT_DC_SHIFT) & RT_DCLS_MASK) * Wn;   // (task-rows mode: the block's first row)
    const u64* rm = a.task_rows ? rc : a.rr + (size_t)(a.n_dc + ((flags >> RT_DM_SHIFT) & RT_DCLS_MASK)) * Wn;
    u32 p0 = 0, p1 = 0, g0 = 0, g1 = 0;
    if (flags & RT_PORTS) {
        p0 = wv::uload(a.pset_off + pset);
        p1 = wv::uload(a.pset_off + pset + 1);
    }
    if (a.n_rg) {
        const u32 gset = wv::uload(a.tg + t);
        g0 = wv::uload(a.gs_off + gset);
        g1 = wv::uload(a.gs_off + gset + 1);
    }
    const u32 ck = a.csi_of ? wv::uload(a.csi_of + t) : R6_NONE;
    const u64* vrow = ck != R6_NONE ? a.vrows + (size_t)ck * Wn : nullptr;
    u32 best = R6_NONE;
    for (u32 w = tid; w < Wn; w += 1024) {
        u64 m = scrow[w] & ~ld(xrow + w);
        if (res) m &= ld(rc + w) & ld(rm + w);
        for (u32 g = g0; g < g1; ++g) m &= ld(a.rg + (size_t)wv::uload(a.gs_row + g) * Wn + w);
        if (vrow) m &= vrow[w];
        for (u32 p = p0; p < p1; ++p) m &= ~ld(a.portmap + (size_t)wv::uload(a.pset_ids + p) * Wn + w);
        u32 rel = 0;
        for (int b = nb - 1; b >= 0; --b) {
            const u64 c = m & ~ld(a.planes + (size_t)b * Wn + w);
            if (c) m = c;
            else if (m) rel |= 1u << b;
        }
        best = min(best, m ? rel : R6_NONE);
    }
    best = wv::min_u32(best);
    if (lane == 0) red[wave] = best;
    wv::barrier();
    u32 gl = R6_NONE;
    for (u32 v = 0; v < 16; ++v) gl = min(gl, red[v]);
    u32 running = 0, at0 = 0;
    u64 c0 = 0;   // this thread's first word: its nodes of the level and their first position
    for (u32 w0 = 0; w0 < Wn; w0 += 1024) {
        const u32 w = w0 + tid;
        u64 c = (w < Wn && gl != R6_NONE) ? a.cbase[w] : 0ull;   // the ready nodes whose level IS gl
        for (int b = 0; b < nb && c; ++b) {
            const u64 pl = ld(a.planes + (size_t)b * Wn + w);
            c &= ((gl >> b) & 1u) ? pl : ~pl;
        }
        const u32 pc = (u32)wv::popc64(c);
        u32 ex = 0, tot = 0;   // the counts (<= 64: seven bits) summed over the lower lanes plane by plane
        WV_UNROLL
        for (u32 bit = 0; bit < 7; ++bit) {
            const u64 bm = wv::ballot(((pc >> bit) & 1u) != 0);
            ex += wv::mbcnt(bm) << bit;
            tot += (u32)wv::popc64(bm) << bit;
        }
        wv::barrier();   // (the counts of the chunk before are read)
        if (lane == 0) red[16 + wave] = tot;
        wv::barrier();
        u32 off = 0, all = 0;
        for (u32 v = 0; v < 16; ++v) {
            const u32 x = red[16 + v];
            off += v < wave ? x : 0u;
            all += x;
        }
        if (w < Wn) {
            a.cmask[w] = c;   // (the words beyond a thread's first are read back below by the thread that wrote them)
            a.crank[w] = running + off + ex;
        }
        if (w0 == 0) { c0 = c; at0 = off + ex; }
        running += all;
    }
    const bool on = running != 0 && running <= r6_compact_cap(Wn);
    if (on)
        for (u32 w = tid; w < Wn; w += 1024) {
            u64 c = w == tid ? c0 : FUSED ? wv::g_fresh64(a.cmask + w) : a.cmask[w];   // (a thread's first word: from its registers, no round trip)
            u32 at = w == tid ? at0 : FUSED ? wv::g_fresh32(a.crank + w) : a.crank[w];
            while (c) {
                a.cidx[at++] = w * 64u + (u32)wv::ffs64(c);
                c &= c - 1ull;
            }
        }
    if (tid == 0) {
        a.blk->csize = on ? running : 0u;
        a.blk->clevel = gl;
    }
}
WV_KERNEL(1024) void k_r6_compact(R6Args a) {
    const u32 t = wv::uload(&a.blk->pos);
    if (t >= wv::uload(&a.blk->end) || wv::uload(&a.blk->error) != ERR_NONE) return;
    r6_compact_body<false>(a, t, reinterpret_cast<u32*>(wv::lds()));   // [16] a wave's minimum, [16] a wave's count
}

// ---- propose: one workgroup of R6_PW waves per task of the block -----------------------------------------------------------
// The waves split the task's node words (wave v owns the chunks of 64 words k = v, v + R6_PW, ...): the passes are latency-bound,
// so more waves per task is what shortens them. A pass ends with one barrier (has any wave a candidate left?).
// (TWB: the largest block the instance's twin count covers — R6_FLAT_BMAX in the instances of the flat rounds, which are the code they
// were before there was a ring; R6_BMAX in the _r instances, which the ring rounds launch)
template <int UN, bool CPT = false, u32 PW = R6_PW, u32 TWB = R6_FLAT_BMAX> WV_DEV void r6_propose_t(const R6Args& a) {
    const u32 lane = wv::lane(), wave = wv::wave();
    const u32 t = wv::uload(&a.blk->pos) + wv::block();
    if (t >= wv::uload(&a.blk->end) || wv::uload(&a.blk->error) != ERR_NONE) return;   // (an error stops the rounds until the host has seen it)
    const RTask* rt = a.rt + t;
    const i64 rcpu = wv::uload(&rt->cpu), rmem = wv::uload(&rt->mem);
    const u32 flags = wv::uload(&rt->flags), svc = wv::uload(&rt->svc), scid = wv::uload(&rt->sc), pset = wv::uload(&rt->pset);
    const u64 maxrep = wv::uload(&rt->maxrep);
    const u32 Wn = a.n_words, KC = r6_chunks(Wn);   // a multiple of UN * PW; the chunks beyond the row hold no candidates
    u64* A = wv::lds();
    u64* Bf = A + (size_t)KC * 64;
    u32* flag = reinterpret_cast<u32*>(Bf + (size_t)KC * 64);   // [R6_NP + 2] "some wave still has a candidate", one word per pass
    const u64* scrow = a.sc + (size_t)scid * Wn;
    const u64* xrow = a.X + (size_t)svc * a.xs;
    const bool res = (flags & RT_RES) != 0;
    // the two demand-class rows of the task — or, in task-rows mode, its own row of this round (twice)
    const u64* rc = a.task_rows ? a.trows + (size_t)wv::block() * Wn : a.rr + (size_t)((flags >> RT_DC_SHIFT) & RT_DCLS_MASK) * Wn;
    const u64* rm = a.task_rows ? rc : a.rr + (size_t)(a.n_dc + ((flags >> RT_DM_SHIFT) & RT_DCLS_MASK)) * Wn;
    u32 p0 = 0, p1 = 0;
    if (flags & RT_PORTS) {
        p0 = wv::uload(a.pset_off + pset);
        p1 = wv::uload(a.pset_off + pset + 1);
    }
    u32 g0 = 0, g1 = 0;   // the task's generic rows
    if (a.n_rg) {
        const u32 gset = wv::uload(a.tg + t);
        g0 = wv::uload(a.gs_off + gset);
        g1 = wv::uload(a.gs_off + gset + 1);
    }
    const u32 ck = a.csi_of ? wv::uload(a.csi_of + t) : R6_NONE;   // a task with cluster mounts: its VolumesFilter row of this round
    const u64* vrow = ck != R6_NONE ? a.vrows + (size_t)ck * a.n_words : nullptr;
    // The task's plain candidates AND the minimum level among them in one pass: lane l of wave v owns words {l + 64 k}, k = v (mod
    // PW); per word the candidate set is narrowed over the level planes from the top in registers (m & ~plane ≠ ∅ ? keep that : the
    // bit is set in the word's minimum), the planes of UN words requested together; the minimum over the words is one reduction.
    // How many tasks of the block in front of this one are IDENTICAL to it (same descriptor): each of them takes — strikes — the first
    // candidate nobody took before it, out of the same set in the same order, so when this task's turn comes the first `twins`
    // candidates of the level are gone whatever the other tasks did. Its list starts behind them (below): a block of one service's
    // tasks then walks 32 half-words PER TASK into the level instead of sharing one window of 32. The ids are requested here and
    // counted behind the pass.
    u32 tw_id[(TWB + 64 * PW - 1) / (64 * PW)], tw_mine = 0;
    const u32 tw_pos = wv::uload(&a.blk->pos);
    if (a.tmpl) {
        tw_mine = wv::uload(a.tmpl + t);
        WV_UNROLL
        for (u32 q = 0; q < (TWB + 64 * PW - 1) / (64 * PW); ++q) {
            const u32 u = tw_pos + (q * PW + wave) * 64 + lane;
            tw_id[q] = u < t ? a.tmpl[u] : R6_NONE;
        }
    }
    const u32 maxrel = wv::uload(&a.blk->maxrel);
    const int nb = 32 - wv::clz32(maxrel);          // planes in use (0: every valid node sits on the base level)
    u32* R = reinterpret_cast<u32*>(Bf);            // [KC * 64] the word's own minimum level above the base, R6_NONE: no candidate in it
    // the round's compact index (R6Args.compact): VW words of positions, the plain half-words are numbered behind them
    const u32 csize = CPT ? wv::uload(&a.blk->csize) : 0u, VW = (csize + 63u) >> 6;
    u64* V = reinterpret_cast<u64*>(R + (size_t)KC * 64);   // [VW <= KC * 16 + 1] the task's candidates by compact position (the upper half of Bf)
    for (u32 i = wave * 64 + lane; i < VW; i += 64 * PW) V[i] = 0;
    u32 best = R6_NONE;
    for (u32 k0 = wave; k0 < KC; k0 += UN * PW) {
        u64 m[UN], f[UN];
        WV_UNROLL
        for (int u = 0; u < UN; ++u) {
            const u32 w = (k0 + u * PW) * 64 + lane;
            const bool in = w < Wn;
            m[u] = in ? scrow[w] : 0ull;
            f[u] = in ? xrow[w] : 0ull;
            if (res && in) f[u] |= ~(rc[w] & rm[w]);
            for (u32 g = g0; g < g1; ++g)
                if (in) f[u] |= ~a.rg[(size_t)wv::uload(a.gs_row + g) * Wn + w];
            if (vrow && in) f[u] |= ~vrow[w];
        }
        u32 rel[UN];
        WV_UNROLL
        for (int u = 0; u < UN; ++u) {
            const u32 w = (k0 + u * PW) * 64 + lane;
            m[u] &= ~f[u];
            for (u32 p = p0; p < p1; ++p)
                if (m[u]) m[u] &= ~a.portmap[(size_t)wv::uload(a.pset_ids + p) * Wn + w];
            rel[u] = 0;
        }
        for (int hi = nb; hi > 0; hi -= 8) {   // eight planes a batch (a batch is all there is below 256 levels)
            const int lo = hi > 8 ? hi - 8 : 0;
            u64 q[UN][8];
            WV_UNROLL
            for (int u = 0; u < UN; ++u) {
                const u32 w = (k0 + u * PW) * 64 + lane;
                // (a word without candidates needs no planes — but on a small node set waiting for m costs more than the loads: there the top
                // batch is requested together with the rows)
                const bool want = (hi == nb && Wn <= 512u) ? w < Wn : m[u] != 0;   // m != 0 only inside the row
                WV_UNROLL
                for (int b = 0; b < 8; ++b) q[u][b] = (lo + b < hi && want) ? a.planes[(size_t)(lo + b) * Wn + w] : 0ull;
            }
            WV_UNROLL
            for (int u = 0; u < UN; ++u) {
                WV_UNROLL
                for (int b = 7; b >= 0; --b) {
                    if (lo + b >= hi) continue;
                    const u64 c = m[u] & ~q[u][b];
                    if (c) m[u] = c;
                    else if (m[u]) rel[u] |= 1u << (lo + b);
                }
            }
        }
        WV_UNROLL
        for (int u = 0; u < UN; ++u) {
            const u32 idx = (k0 + u * PW) * 64 + lane;
            A[idx] = m[u];
            const u32 r = m[u] ? rel[u] : R6_NONE;
            R[idx] = r;
            best = min(best, r);
        }
    }
    best = wv::min_u32(best);
    u32 tw_cnt = 0;
    if (a.tmpl) {
        WV_UNROLL
        for (u32 q = 0; q < (TWB + 64 * PW - 1) / (64 * PW); ++q) tw_cnt += (u32)wv::popc64(wv::ballot(tw_id[q] == tw_mine && tw_pos + (q * PW + wave) * 64 + lane < t));
    }
    if (lane == 0) {
        flag[wave] = best;
        flag[PW + wave] = tw_cnt;
    }
    wv::barrier();
    u32 gmin = R6_NONE, twins = 0;
    for (u32 v = 0; v < PW; ++v) {
        gmin = min(gmin, flag[v]);
        twins += flag[PW + v];
    }
    const u32 level = gmin == R6_NONE ? R6_NONE : wv::uload(&a.blk->base) + gmin;
    // the task's minimum level is the compact index's: its candidates are among the index's nodes; every wave moves those of its share of
    // the words to their positions
    const bool cmode = CPT && csize != 0 && gmin == wv::uload(&a.blk->clevel);
    if (CPT && cmode) {
        u32* V32 = reinterpret_cast<u32*>(V);
        for (u32 idx = wave * 64 + lane; idx < Wn; idx += 64 * PW) {
            u64 m = R[idx] == gmin ? A[idx] : 0ull;
            if (!m) continue;
            const u64 cm = a.cmask[idx];
            const u32 r0 = a.crank[idx];
            while (m) {
                const u64 low = m & (0ull - m);
                const u32 vp = r0 + (u32)wv::popc64(cm & (low - 1ull));
                wv::lds_or32(V32 + (vp >> 5), 1u << (vp & 31u));
                m ^= low;
            }
        }
        wv::barrier();
    }
    if (wave != 0) return;   // (every wave is past the last barrier) wave 0 lists the candidates and writes the proposal
    const u32 nw = cmode ? VW : Wn, hw_off = cmode ? 0u : 2u * VW;
    R6Prop* out = a.prop + wv::block();
    // its first non-empty half-words, in node order (what the matcher walks: a word that is half empty does not cost a list entry):
    // 64 words a step, a lane's place in the list = the non-empty half-words in front of it (two ballots)
    // (an _r instance runs ring rounds only — launch_r6_rounds — and a ring round has an extension: its records are R6PropExtRing)
    constexpr bool RINGP = R6_RING_ON && TWB > R6_FLAT_BMAX;
    using Ext = typename std::conditional<RINGP, R6PropExtRing, R6PropExt>::type;
    Ext* ext = a.ext ? reinterpret_cast<Ext*>(a.ext) + wv::block() : nullptr;
    const u32 lmax = ext ? (RINGP ? (u32)R6_LIST_RING : (u32)R6_LIST) : 2u * R6_CAND;
    u32 cnt = 0, more = 0;
    u32 skip = twins, last_hw = 0, last_hb = 0;   // candidates still to pass over; the last non-empty half-word passed over
    u32 h0 = R6_NONE;   // the half-word of the level's first candidate, the twins' share included (the second section ends in front of its word)
    // the non-empty halves (lo, hi) of the lanes' words of chunk k go to the list behind its `cnt` entries, in lane order
    auto put = [&](u32 k, u32 lo, u32 hi, u64 b_lo, u64 b_hi) {
        const u32 at_lo = cnt + wv::mbcnt(b_lo) + wv::mbcnt(b_hi), at_hi = at_lo + (lo != 0 ? 1u : 0u);
        if (lo && at_lo < 2 * R6_CAND) {
            out->hw[at_lo] = (unsigned short)(hw_off + 2 * (k * 64 + lane));
            out->hb[at_lo] = lo;
        } else if (lo && at_lo < lmax) {
            ext->hw[at_lo - 2 * R6_CAND] = (unsigned short)(hw_off + 2 * (k * 64 + lane));
            ext->hb[at_lo - 2 * R6_CAND] = lo;
        }
        if (hi && at_hi < 2 * R6_CAND) {
            out->hw[at_hi] = (unsigned short)(hw_off + 2 * (k * 64 + lane) + 1);
            out->hb[at_hi] = hi;
        } else if (hi && at_hi < lmax) {
            ext->hw[at_hi - 2 * R6_CAND] = (unsigned short)(hw_off + 2 * (k * 64 + lane) + 1);
            ext->hb[at_hi - 2 * R6_CAND] = hi;
        }
        const u32 total = cnt + (u32)wv::popc64(b_lo) + (u32)wv::popc64(b_hi);
        if (total > lmax) more = 1;
        cnt = min(total, lmax);
    };
    if (level != R6_NONE)
        for (u32 k = 0; k < (nw + 63u) / 64u && !more; ++k) {   // (the chunks beyond the row hold nothing)
            const u64 m = cmode ? (k * 64 + lane < VW ? V[k * 64 + lane] : 0ull) : (R[k * 64 + lane] == gmin ? A[k * 64 + lane] : 0ull);   // the words whose own minimum is the task's
            u32 lo = (u32)m, hi = (u32)(m >> 32);
            u64 b_lo = wv::ballot(lo != 0), b_hi = wv::ballot(hi != 0);
            if (!(b_lo | b_hi)) continue;
            if (R6_LEVELS2 && !CPT && h0 == R6_NONE) {
                const u32 fl = (u32)wv::ffs64(b_lo | b_hi);
                h0 = 2 * (k * 64 + fl) + (((b_lo >> fl) & 1ull) ? 0u : 1u);
            }
            if (skip) {
                // candidates in front of a lane's word: the popcounts (<= 64: seven bits) summed over the lower lanes plane by plane
                const u32 pl = (u32)wv::popc64((u64)lo), pc = pl + (u32)wv::popc64((u64)hi);
                u32 ex = 0, tot = 0;
                WV_UNROLL
                for (u32 bit = 0; bit < 7; ++bit) {
                    const u64 bm = wv::ballot(((pc >> bit) & 1u) != 0);
                    ex += wv::mbcnt(bm) << bit;
                    tot += (u32)wv::popc64(bm) << bit;
                }
                // a half-word whose candidates ALL lie among the first `skip` is passed over (the others keep their struck bits: the
                // matcher meets them in the TK row)
                const bool drop_lo = ex + pl <= skip, drop_hi = ex + pc <= skip;
                const u64 gone = wv::ballot(pc != 0 && drop_hi);   // words passed over entirely ...
                const u64 half = wv::ballot(lo != 0 && drop_lo && !(pc != 0 && drop_hi));   // ... and the one word whose low half alone is
                if (gone | half) {   // remember the last half-word passed over: a level with no more than `skip` candidates lists that one
                    const u32 lg = gone ? 63u - (u32)__builtin_clzll(gone) : 0u, lh = half ? 63u - (u32)__builtin_clzll(half) : 0u;
                    if (half && (!gone || lh > lg)) {
                        last_hw = hw_off + 2 * (k * 64 + lh);
                        last_hb = wv::readlane(lo, lh);
                    } else {
                        const u32 hi_l = wv::readlane(hi, lg), lo_l = wv::readlane(lo, lg);
                        last_hw = hw_off + 2 * (k * 64 + lg) + (hi_l ? 1u : 0u);
                        last_hb = hi_l ? hi_l : lo_l;
                    }
                }
                if (drop_lo) lo = 0;
                if (drop_hi) hi = 0;
                skip = tot <= skip ? skip - tot : 0u;
                b_lo = wv::ballot(lo != 0);
                b_hi = wv::ballot(hi != 0);
                if (!(b_lo | b_hi)) continue;
            }
            put(k, lo, hi, b_lo, b_hi);
        }
    // ---- the second section (R6Args.levels2): where a lap over the node set ends, one class of tasks after the other finds every node
    // of its minimum level L taken; what such a task wants then is the first node of level L + 1 that passes its filters, and at propose
    // time that is known. A COMPLETE level-L listing (not cut by the list's length, the twins' share below the level's candidates) of a
    // task without cluster mounts goes on with the first non-empty half-words, in node order, of the task's plain candidates on level
    // EXACTLY L + 1 that lie in words in front of h0's — the half-word of the level's first candidate, the twins' share included — as
    // far as the list has room (bit 31 of n_cand: the room cut the section). R6Prop.level stays L. Exact, because
    //   * inside a block levels only grow and feasibility only shrinks: no candidate on a level <= L ever appears, so once the first
    //     section is dead the task's candidates on L + 1 are nodes that were on L + 1 at propose time and nodes the block moved up from L;
    //   * a node moved up that passes the task's filters was one of its level-L candidates: it lies in a half-word >= h0, behind every
    //     entry of the section — and so does every L + 1 node the section left out. A live listed entry beats them all;
    //   * a listed node whose TK bit is clear is as the propose saw it: no task of the block was placed on it, X of the service moves on
    //     taken nodes only (volumes are the one cluster-wide state: tasks with mounts get no section); one a crossing task took is struck
    //     like any other (its TK bit stays set, it moved to L + 2);
    //   * L + 1 exactly: on a higher level a node moved up to L + 1 would win whatever its index. Beyond Blk6.maxrel there is nothing to list;
    //   * a section that is empty or runs dry cuts the block, as a list of one level does. A cut is always allowed.
    // Nothing is loaded: the first pass left every word's candidates on the WORD's minimum level in A and that level in R, and a word
    // in front of h0's has no candidate on L — its minimum is L + 1 or it holds none of that level. (The low half of h0's own word, when h0
    // is a high half, is left out with everything behind it: its L + 1 candidates are not in A.) Entries are (half-word, bits) pairs
    // to the commit kernel, which walks them in list order: the two sections never share a half-word, their bit sets are disjoint.
    u32 first_len = cnt;
    if (R6_LEVELS2 && !CPT && a.levels2 && level != R6_NONE && !more && cnt != 0 && cnt < lmax && ck == R6_NONE && gmin < maxrel && h0 != R6_NONE) {
        const u32 w_end = h0 >> 1;   // (0: the level's first candidate sits in word 0, no section)
        for (u32 k = 0; k * 64 < w_end && !more; ++k) {
            const u32 idx = k * 64 + lane;
            const u64 m = (idx < w_end && R[idx] == gmin + 1u) ? A[idx] : 0ull;
            const u32 lo = (u32)m, hi = (u32)(m >> 32);
            const u64 b_lo = wv::ballot(lo != 0), b_hi = wv::ballot(hi != 0);
            if (b_lo | b_hi) put(k, lo, hi, b_lo, b_hi);
        }
        if ((a.dbg & 16u) && cnt > first_len && lane == 0) r6_count32(&a.blk->dbg_lv2);
    }
    // no plain candidate: the service's exception list by the full key (scheduler.go:708-735), lanes stride over the entries
    u64 bhi = KEY_NONE, blo = KEY_NONE;
    u32 be = 0;
    const u32 e0 = wv::uload(a.list_off + svc), e1 = level == R6_NONE ? wv::uload(a.list_off + svc + 1) : e0;
    for (u32 e = e0 + lane; e < e1; e += 64) {
        const u32 n = a.list_node[e];
        if (n == LIST_EMPTY) continue;
        const u32 w = n >> 6;
        const u64 bit = 1ull << (n & 63);
        if (!(scrow[w] & bit)) continue;
        if (res && !(rcpu <= a.cpu[n] && rmem <= a.mem[n])) continue;
        bool lacks = false;   // HasEnough per reservation, validate.go:24-52
        for (u32 g = g0; g < g1; ++g) {
            const u32 r = a.gs_row[g];
            if (a.gcnt[(size_t)a.rg_kind[r] * a.gstride + n] < a.rg_val[r]) lacks = true;
        }
        if (lacks) continue;
        if (vrow && !(vrow[w] & bit)) continue;
        bool used = false;
        for (u32 p = p0; p < p1; ++p)
            if (a.portmap[(size_t)a.pset_ids[p] * Wn + w] & bit) used = true;
        if (used) continue;
        const u32 sv = a.list_svc[e], fl = a.list_fail[e];
        if ((flags & RT_MAXREP) && !((u64)sv < maxrep)) continue;   // filter.go:373-375
        const u32 fcl = fl >= MAX_FAILURES ? fl - (MAX_FAILURES - 1) : 0u;
        const u64 hi = ((u64)fcl << 32) | sv, lo = ((u64)a.total[n] << 32) | n;
        if (hi < bhi || (hi == bhi && lo < blo)) {
            bhi = hi;
            blo = lo;
            be = e;
        }
    }
    const u64 ghi = r6_wave_min64(bhi);
    const u64 glo = r6_wave_min64(bhi == ghi ? blo : KEY_NONE);
    const u64 who = wv::ballot(bhi == ghi && blo == glo && ghi != KEY_NONE);
    const u32 gentry = who ? wv::readlane(be, (u32)wv::ffs64(who)) : 0u;
    if (level != R6_NONE && cnt == 0) {   // every candidate of the level lies among the twins' share: the level's last half-word, all taken by then (a cut)
        if (lane == 0) {
            out->hw[0] = (unsigned short)last_hw;
            out->hb[0] = last_hb;
        }
        cnt = 1;
    }
    if (lane >= cnt && lane < 2 * R6_CAND) {
        out->hw[lane] = 0;
        out->hb[lane] = 0;
    }
    if (lane == 0) {
        out->level = level;
        out->n_cand = cnt | (more ? 0x80000000u : 0u);
        out->exc_hi = ghi;
        out->exc_lo = ghi == KEY_NONE ? KEY_NONE : glo;
        out->exc_entry = gentry;
        out->flags = ((flags & RT_UNCOUNTED) ? 1u : 0u) | (ck != R6_NONE ? 2u : 0u);
    }
}

// (UN follows the node set: r6_unroll(n_words); the shard drivers' ranges may differ in size, so they pass it per range)
WV_DEV void r6_propose(const R6Args& a) {
    if (a.n_words <= R6_SMALL_WORDS) r6_propose_t<1>(a);
    else r6_propose_t<R6_UNROLL>(a);
}
WV_KERNEL(64 * R6_PW) void k_r6_propose(R6Args a) { r6_propose(a); }
WV_KERNEL(64 * R6_PW) void k_r6_propose_small(R6Args a) { r6_propose_t<1>(a); }   // n_words <= R6_SMALL_WORDS only: the registers of ONE chunk
// n_words <= R6_TINY_WORDS only: four waves a task, each with one chunk — half the threads, so that the workgroups of a block of 1 408
// are all resident at once (8 to a CU); at 157 node words three of eight waves had a word at all
WV_KERNEL(64 * R6_PW_TINY) void k_r6_propose_tiny(R6Args a) { r6_propose_t<1, false, R6_PW_TINY>(a); }
#if R6_RING_ON
// ... the instances of the ring rounds (R6Args.ring): a twin count over blocks of up to R6_BMAX tasks, lists of up to R6_LIST_RING half-words
WV_KERNEL(64 * R6_PW) void k_r6_propose_r(R6Args a) {
    if (a.n_words <= R6_SMALL_WORDS) r6_propose_t<1, false, R6_PW, R6_BMAX>(a);
    else r6_propose_t<R6_UNROLL, false, R6_PW, R6_BMAX>(a);
}
WV_KERNEL(64 * R6_PW) void k_r6_propose_small_r(R6Args a) { r6_propose_t<1, false, R6_PW, R6_BMAX>(a); }
WV_KERNEL(64 * R6_PW_TINY) void k_r6_propose_tiny_r(R6Args a) { r6_propose_t<1, false, R6_PW_TINY, R6_BMAX>(a); }
#endif
// ... the instances that honour a round's compact index (launched behind k_r6_compact only)
WV_KERNEL(64 * R6_PW) void k_r6_propose_c(R6Args a) {
    if (a.n_words <= R6_SMALL_WORDS) r6_propose_t<1, true>(a);
    else r6_propose_t<R6_UNROLL, true>(a);
}
WV_KERNEL(64 * R6_PW) void k_r6_propose_small_c(R6Args a) { r6_propose_t<1, true>(a); }

// index of the first of n ascending thresholds that is greater than q (n: none)
WV_DEV u32 r6_first_above(const i64* thr, u32 n, i64 q) {
    u32 lo = 0, hi = n;
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (thr[mid] > q) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// ---- commit: match the block in task order (wave 0), then apply the accepted picks (all threads) ---------------------------
// (CSI: the instance for batches with cluster mounts — choosing volumes indexes a small array dynamically, which costs the kernel a scratch
// segment; the ordinary instances have none)
// (R7: the instance of the node-range shards, swp_resolve7.hpp — the same kernel on every shard: a thread FOLDS the proposals all shards
// made for its task into one list in global node order while it stages it, wave 0 matches the block exactly as below — every shard
// computes the same picks —, and a pick is applied by the shard that owns its node. m7 / my: the other shards' proposals, this shard's number.)
// (RING: the ring instance, k_r6_commit_r — R6Args.ring != 0, no compact index, no cluster mounts, no runs-by-rank path. Pick slots and
// windows are indexed by task % ring with `ring` as the row stride: RS below. Every other instance has RS == a.block and slot == task.)
template <bool CPT, bool CSI, bool R7 = false, bool RING = false> WV_DEV void r6_commit_t(const R6Args& a, const R7Args* m7 = nullptr, u32 my = 0) {
    static_assert(!RING || (!CPT && !CSI && !R7), "the ring is the plain instance's");
    const u32 tid = wv::tid(), lane = wv::lane();
    const u32 pos = a.blk->pos, end = a.blk->end;
    if (pos >= end || a.blk->error != ERR_NONE) return;   // a level beyond the planes: the proposals of this round were not written
    if constexpr (R7) {
        if (r7_any_dead(m7)) return;
    }
    const u32 n = min(a.block, end - pos), Wn = a.n_words, n_rr = a.n_dc + a.n_dm;
    // (with a compact index the positions' words come first, the node words behind them: addresses as the lists carry them)
    // (R7: the TK row covers the padded half-word space of ALL shards)
    const u32 VW = CPT ? (a.blk->csize + 63u) >> 6 : 0u;
    u32 tkw = CPT ? r6_tk_words(Wn) : Wn;
    if constexpr (R7) tkw = r7_tk_words(m7);
    const u32 rnd = a.blk->rounds;   // (R7: the same on every shard — the parity of the trailer slots)
    u64* tk = wv::lds();                                         // [tkw] addresses taken by this block so far
    i64* thr = reinterpret_cast<i64*>(tk + tkw);                 // [n_rr] the demand-class thresholds
    // RING — the slot of 64 tasks that group g uses is g % 15's, the slot of helper g % 15. Reuse is safe, writer by writer:
    //   * L_hw / L_hb / L_cur of slot s: written by the prologue (waves 0 and 1, groups 0 and 1 into slots 0 and 1, in front of their publish
    //     of staged[0 / 1]) and by helper s alone, in its stage() and its cursor loop. A helper takes its groups g, g + 15, ... in order and
    //     stages group g + 15 at the top of its loop, BEHIND its apply of group g; it applied g behind the matcher's publish of g's picks
    //     (sh[3] >= the group's end). The matcher reads a slot only between its acquire of staged[g] and its publish of group g's picks —
    //     its ah / ab registers live inside one group, and the release of that publish waits for every LDS read it has in flight — so it
    //     is done with slot s for group g before helper s writes it for g + 15, and reads it for g + 15 only behind the acquire of
    //     staged[g + 15], which helper s publishes behind its last stage() of that group.
    //   * pk_node / pk_idx / pk_aux of slot s: written by the matcher for group g in front of its publish of g's picks, read by helper s in
    //     its apply of g; the matcher writes them for g + 15 behind its acquire of staged[g + 15], which helper s published behind that
    //     apply. The runs-by-rank path, whose scratch is a group's pick slots, is off in this instance.
    //   * a block cut inside group g: helper g % 15 leaves its loop behind its apply; nobody stages a later group (a helper that finds
    //     the matching over leaves without a publish), and the matcher's loop has ended.
    // The TK row is per node, not per task: it holds every pick of the block, and windows are staged against it as ever.
    const u32 RS = RING ? a.ring : a.block;                      // row stride of the pick and window arrays
    u32* pk_node = reinterpret_cast<u32*>(thr + n_rr);           // [RS] node, R6_NONE = no suitable node
    u32* pk_idx = pk_node + RS;                                  // [RS] commit index / index among the unplaceable tasks
    u32* pk_aux = pk_idx + RS;                                   // [RS] exception-list entry (LIST_EMPTY: plain node) / commits before an unplaceable task
    u32* sh = pk_aux + RS;                                       // [0] accepted, [1] ncommit, [2] ninf, [3] tasks decided so far, [4] the matching is over
    u32* staged = sh + 16;                                       // [R6_FLAT_BMAX / 64; RING: r6_ring_flags(block)] group g's lists are in LDS
    const u32 n_flags = RING ? r6_ring_flags(a.block) : 32u;
    // The lists in LDS, LW entries a task. R7: the whole folded list, staged by the prologue. Otherwise a WINDOW: the first `win` entries
    // that are live when the task's group is staged — groups 0 and 1 by the prologue (nothing is taken yet: the list's first entries),
    // group g >= 2 by the wave that will apply it, against the TK row once the matcher has published the picks of group g - 2. Taken
    // nodes stay taken, so what is dead then is dead; what dies later meets the seating step's own TK test. A task whose window runs
    // out while entries were left out of it is treated as one whose list is exhausted: the block is cut in front of it (a cut is
    // always allowed) and counted in Blk6.cut_window.
    // (R6Args.win: the engine gives batches of long runs of identical tasks windows of 2 * R6_CAND in blocks of 768 — the runs-by-rank path
    // takes a whole run from ONE task's window, and service-major cfg3 lost a fifth with windows of 16)
    constexpr u32 LMAX = 2u * R6_CAND;
    const u32 LW = R7 ? LMAX : r6_win_of(a.win);   // rows of the two arrays
    const u32 win = (R7 || !((a.dbg >> 12) & 31u)) ? LW : min((a.dbg >> 12) & 31u, LW);   // (dbg bits 12-16: a shorter window, tests)
    u32* L_hb = sh + 16 + n_flags;                               // [LW][RS] entry-major: lane i of the matcher reads
    u32* L_cur = L_hb + (size_t)LW * RS;                         // ... entry k of the task in slot i at [k * RS + i] (no bank conflicts); [RS] a lower bound of every task's cursor: the entries in front of it are dead
                                                                 // (not R7: | entries in the window << 8 | R6C_LEFT | the head's bits, R6C_*)
    unsigned short* L_hw = reinterpret_cast<unsigned short*>(L_cur + RS);   // [LW][RS] the half-word indices, 16 bits each (the engine refuses node sets beyond 2^21 nodes)
    u32* H_level = reinterpret_cast<u32*>(L_hw + (size_t)LW * a.block);   // R7 only: [block] the folded record's level ...
    u32* H_meta = H_level + a.block;                                       // ... and its list length | R7M_* flags
    for (u32 j = tid; j < RS; j += R6_COMMIT_THREADS) L_cur[j] = 0;
    for (u32 w = tid; w < (R7 ? tkw : Wn + VW); w += R6_COMMIT_THREADS) tk[w] = 0;
    for (u32 c = tid; c < n_rr; c += R6_COMMIT_THREADS) thr[c] = a.thr[c];
    if (tid < n_flags) staged[tid] = 0;
    // Wave v >= 1 applies the picks of the block's groups v - 1, v + 14, ... (group g: tasks 64 g ...) as soon as wave 0 has matched the
    // group, while it matches the next ones; the first group's task records are requested now. (R7: a block has sixteen groups at most,
    // and the last one is applied by wave 0 behind its matching.)
    const u32 wave_ = wv::wave();
    const u32 mine0 = wave_ == 0 ? (R7 ? 15u * 64u + lane : R6_NONE) : (wave_ - 1u) * 64u + lane;   // the first block-local task this thread applies
    RTask r0{};
    if (mine0 < n) r0 = a.rt[pos + mine0];
    if (tid == 0) { sh[3] = 0; sh[4] = 0; }
    if constexpr (R7 && CSI) {
        if (tid == 0) sh[12] = r7_take_trailers(a, m7, my, rnd);   // the volumes the other shards reserved in the round before: into this shard's table
    }
    const bool prof = (a.dbg & 16u) != 0;
    const u64 t0 = prof ? wv::clock64() : 0;
    const bool runs_on = !R7 && !RING && a.tmpl != nullptr && a.no_runs == 0;   // the runs-by-rank path below
    u64 exc0_lo = 0;      // thread 0: the exception-list candidate of the block's first task, the only one that may use its own
    u32 exc0_entry = 0;
    wv::barrier();
    // every thread stages the lists of its task (wave g: the block's group g): the matcher walks them with a cursor (an entry is looked
    // at once) instead of holding all of them in registers. No barrier: a group's flag is published when its lists are in LDS.
    if constexpr (R7) {
        // A few folds at a time, in group order: a fold is three dependent batches of uncoalesced loads, and the batches of eleven waves
        // queue up in the CU's one address path — the matcher's own group (wave 0 stages it) then waits behind all the others': 27.8 k
        // cycles before the matching starts. Alone a fold takes 11.9 k (latency bound), but then the chain is slower than the matcher
        // (a group is matched in ≈ 11 k): measured on cfg4 200k x 40k over 4 / 8 shards, window 1: 33.6 / 45.1 ms, 2: 29.8 / 38.1,
        // 4: 30.1 / 37.2, all at once: 30.9 / 38.4. (Between GPUs a batch takes longer — peer reads — so rather more in flight than fewer.)
        const u32 fw = ((a.dbg >> 8) & 15u) ? ((a.dbg >> 8) & 15u) : R7_FOLDS_IN_FLIGHT;
        if (wave_ >= fw)
            while (wv::lds_poll32(staged + (wave_ - fw)) == 0) wv::spin_pause();
        if ((tid & ~63u) < n) r7_fold_into(m7, tid < n ? tid : 0u, tid < n, a.block, L_hw, L_hb, H_level, H_meta, sh);   // (whole waves: it ballots)
    } else {
        // (waves 0 and 1: the block's first two groups, whose window is the front of the list; two waves' uncoalesced loads share the CU's
        // one address path well — with all sixteen at it the matcher's own group queued behind the others')
        if (wave_ < 2u && tid < n) {
            const R6Prop* q = a.prop + tid;
            const u32 lv = q->level, nc = q->n_cand, fl = q->flags;
            const u64 xh = q->exc_hi;
            const u32 tm = runs_on ? a.tmpl[pos + tid] : 0u;
            if (tid == 0) {
                exc0_lo = q->exc_lo;
                exc0_entry = q->exc_entry;
            }
            const u32 total = lv != R6_NONE ? (nc & 0x7FFFFFFFu) : 0u, cnt = min(total, win);
            const u32* qh = reinterpret_cast<const u32*>(q->hw);   // (two indices a dword)
            u32 vh[LMAX / 2], vb[LMAX];   // (all requested together, whatever the list's length: a load under a predicate of its own waits for the one before it)
            WV_UNROLL
            for (int k = 0; k < (int)LMAX / 2; ++k) vh[k] = qh[k];
            WV_UNROLL
            for (int k = 0; k < (int)LMAX; ++k) vb[k] = q->hb[k];
            WV_UNROLL
            for (int k = 0; k < (int)LMAX; ++k)
                if ((u32)k < win) {   // (behind the list's end: index 0 — the seating step reads an entry's TK word before it knows whether the entry counts)
                    L_hw[(size_t)k * RS + tid] = (u32)k < cnt ? (unsigned short)((k & 1) ? vh[k >> 1] >> 16 : vh[k >> 1] & 0xFFFFu) : (unsigned short)0;
                    L_hb[(size_t)k * RS + tid] = vb[k];
                }
            L_cur[tid] = (cnt << 8) | ((lv != R6_NONE && (total > cnt || (nc >> 31))) ? R6C_LEFT : 0u) | r6_head_bits(lv, xh, fl);
            if (runs_on) pk_idx[tid] = tm;   // the task's descriptor id, in its own pick slot: nobody reads the slot before the group is matched
        }
    }
    if (R7 || wave_ < 2u) {
        wv::lockstep();
        if (lane == 0) wv::lds_publish32(staged + wave_, 1u);
    }
    const u64 t1 = prof ? wv::clock64() : 0;
    u32 reseats = 0, seat_steps = 0, late_runs = 0;
    u64 cy_load = 0, cy_walk = 0, cy_g0 = 0, cy_g1 = 0, cy_g2 = 0, cy_h0 = 0, cy_h1 = 0, cy_h2 = 0, cy_s0 = 0, cy_s1 = 0, cy_s2 = 0;
    u32 walks = 0;
    if (wave_ == 0) {
        u32 nc = a.ctl->ncommit, ni = a.ctl->ninf, acc = 0, why = 0;
        u32* tk32 = reinterpret_cast<u32*>(tk);   // the same row as 32-node half-words
        bool stop = false, csi_seen = false;   // csi_seen: a task with cluster mounts is decided in this block already
        // The scalar part of a task's record (level, list length, exception-list candidate, flags) comes from LDS once the group is staged,
        // read behind the wait below: the staging wave left it in the task's L_cur word (R6C_*) and, the descriptor id, in its pk_idx
        // slot — no global load between two walks. (Until the heads moved there wave 0 requested every group's records itself, two groups
        // ahead: six uncoalesced loads a lane in the CU's one address path, next to the helpers' staging loads.)
        // (R7: the folded heads; only the block's first task may use its exception-list candidate, whose record its staging thread left
        // in sh[8..10] — the single engine's thread 0 keeps it from its prologue load)
        struct Head { u32 level, n_cand; u64 exc_hi; u32 flags; };
        auto head7 = [&](u32 j) {
            const u32 mt = H_meta[j];
            return Head{H_level[j], mt & 0xFFu, (mt & R7M_EXC) ? 0ull : KEY_NONE, ((mt & R7M_UNC) ? 1u : 0u) | ((mt & R7M_CSI) ? 2u : 0u)};
        };
        if (R7 && CSI && sh[12]) csi_seen = true;   // a reservation arrived from another shard only now: the proposals of tasks with mounts were made without it
        u32 sg = 0;   // the group's slot: its first task's place in the pick and window arrays (RING: g0 % ring; g0 otherwise)
        for (u32 g0 = 0; g0 < n && !stop; g0 += 64, sg = (RING && sg + 64u >= RS) ? 0u : sg + 64u) {
            const u32 i = g0 + lane, glim = min(64u, n - g0), si = sg + lane;
            const bool have = i < n;
            const u64 tg0 = prof ? wv::clock64() : 0;
            while (wv::lds_poll32(staged + (g0 >> 6)) == 0) wv::spin_pause();   // (long there, but for the first groups of a block)
            const u64 tga = prof ? wv::clock64() : 0;
            const u32 lcur = have ? L_cur[si] : 0u;   // (the group's applying wave has skipped the dead entries so far)
            // the task's descriptor id (a RUN of identical tasks: below) — in a register before the run path uses the group's pick slots as scratch
            const u32 tmid = (runs_on && have) ? pk_idx[si] : 0u;
            if (prof) wv::keep(lcur ^ tmid);   // (the timer below: behind the wait for both)
            const u64 th0 = prof ? wv::clock64() : 0;
            // (a window may be empty — every entry was dead when it was staged — where the list is not: the task is still a plain one)
            u32 nent = (lcur >> 8) & 0xFFu, tflags = (lcur / R6C_UNC) & 3u;   // tflags: R6Prop.flags
            bool plain = (lcur & R6C_PLAIN) != 0;
            bool exc = !plain && (lcur & R6C_EXC) != 0;
            const u32 left_out = R7 ? 0u : (lcur / R6C_LEFT) & 1u;
            if constexpr (R7) {
                const Head rec = head7(have ? i : 0u);
                const u32 level = have ? rec.level : 0u;
                nent = (have && level != R6_NONE) ? (rec.n_cand & 0x7FFFFFFFu) : 0u;
                plain = nent != 0;
                exc = have && level == R6_NONE && rec.exc_hi != KEY_NONE;
                tflags = rec.flags;
            }
            const bool inf = have && !plain && !exc;
            // Every lane carries two half-words of its list — the current one (bits, w) and the next one with a candidate left
            // (bits2, w2), which it steps to inside the walk — and a cursor behind them. An entry is looked at ONCE, against the TK
            // row as it is then (the picks of the earlier groups, and of this group's tasks in front of a stop): what it finds empty
            // stays empty, what it seats is struck by the walk from then on.
            u32 bits = 0, w = 0, bits2 = 0, w2 = 0, cur = R7 ? lcur : lcur & 0xFFu;
            // (straight-line: every lane reads R6_SEAT entries — clamped to its list, the unused entries of a list are zero — and the TK
            // words behind them, the seats are filled by selects: a step is two LDS round trips — one with R6_SEAT_AHEAD, below — and no divergent branch. An entry is
            // consumed while a seat is free; the first one that finds none stays for the next visit, and so do those behind it)
            const u32 li = have ? i : 0u;
            const u32 ls = RING ? (have ? si : sg) : li;   // the lane's column of the window arrays (RING, a lane without a task: the group's first, never another group's slot)
            // R6_SEAT_AHEAD: the entries at the cursor (ah, ab) are requested whenever the cursor has a new value — behind the group's
            // L_cur word and at the end of every seating step — and not waited for: they are in their registers by the time the walk
            // stops, so a stop starts with the TK reads, issued right behind its flush (one LDS round trip of a lone wave among sixteen
            // instead of two, and no address arithmetic). What is read early is what would be read at the stop:
            //   * `cur` moves only in the seating step, which requests the entries again behind it;
            //   * the window of a task (its column of L_hw / L_hb) is written by ONE thread, in front of the publish of staged[group]:
            //     the prologue (waves 0 and 1, or r7_fold_into — the R7 instance's threads write only their own task's column), or the
            //     helper's stage(), every call of which lies in front of its `lds_publish32(staged + g, 1u)`. Behind the publish that
            //     helper's cursor loop writes L_cur[j] alone (and so does the R7 waves'), the run path's scratch is the group's PICK slots
            //     (pk_node / pk_idx / pk_aux), the apply reads pk_* and writes global memory, and the fused compact body starts behind
            //     two barriers that follow the matching. Wave 0 reads a column only behind its acquire of staged[group].
            // A lane that does not `go` at a stop ignores its pair, as it ignored what it loaded there.
            u32 ah[R6_SEAT] = {}, ab[R6_SEAT] = {};
            auto ahead = [&]() {
                WV_UNROLL
                for (int q = 0; q < R6_SEAT; ++q) {
                    const u32 c = min(cur + (u32)q, win - 1u);
                    R6_REACH(R6R_CLAMPED, have && cur + (u32)q > win - 1u && cur < nent);
                    ah[q] = L_hw[c * RS + ls];
                    ab[q] = L_hb[c * RS + ls];
                }
            };
            if (R6_SEAT_AHEAD) ahead();
            auto seat = [&](bool want) {   // lanes with `want` fill their free seats from their cursor on
                bool go = want && bits2 == 0 && cur < nent;
                if (!wv::ballot(go)) return;
                // (one step; more only as long as a lane has NO seat — a second optional step costs more than the stops it saves. The
                // loop is tested at its END, behind the request for the next pair: on the way out nothing waits for that request)
                for ([[maybe_unused]] u32 step = 0;; ++step) {
                    ++seat_steps;
                    R6_REACH(R6R_SECOND_STEP, step >= 1 && lane == 0);
                    R6_REACH(R6R_AT_NENT, want && have && cur >= nent);
                    u32 h[R6_SEAT], b[R6_SEAT], t[R6_SEAT];
                    if (!R6_SEAT_AHEAD) ahead();
                    WV_UNROLL
                    for (int q = 0; q < R6_SEAT; ++q) {
                        h[q] = ah[q];
                        b[q] = ab[q];
                    }
                    WV_UNROLL
                    for (int q = 0; q < R6_SEAT; ++q) t[q] = tk32[h[q]];
                    bool open = go;
                    u32 adv = 0;
                    WV_UNROLL
                    for (int q = 0; q < R6_SEAT; ++q) {
                        open = open && cur + (u32)q < nent && bits2 == 0;
                        const u32 c = open ? b[q] & ~t[q] : 0u;
                        const bool first = bits == 0;
                        bits2 = (c && !first) ? c : bits2;
                        w2 = (c && !first) ? h[q] : w2;
                        w = (c && first) ? h[q] : w;
                        bits = (c && first) ? c : bits;
                        adv += open ? 1u : 0u;
                    }
                    cur += adv;
                    if (R6_SEAT_AHEAD) {   // (every lane: one that did not move asks for the same pair again)
                        R6_SCHED_FENCE();  // (behind the selects, which read the old pair: requested above them the new pair needs registers of its own and a copy — a wait — at the loop's end)
                        ahead();
                    }
                    go = want && bits2 == 0 && cur < nent;
                    if (!wv::ballot(go && bits == 0)) break;
                }
            };
            // ---- A group that is ONE RUN of identical tasks (service-major batches: a service's tasks follow each other) needs no walk.
            // Identical tasks have the same candidates in the same order, and each takes the first one nobody took: task j of the run
            // takes the (j + 1)-th candidate that is still free when the group starts — of lane 0's list, which starts in front of all
            // the others' (a twin's list starts a twin's share further on: k_r6_propose; the candidates in front of lane 0's are taken
            // by then). Lane h looks at entry h of that list behind its cursor and counts what the TK row leaves of it; a prefix sum
            // places the half-words on the lanes' ranks (a marker at every half-word's first rank, summed up: the half-word a rank
            // falls into); every lane picks its bit. If the list holds fewer free candidates than the group has tasks, the ordinary
            // seating and walk take over (they cut the block where the list is exhausted).
            // (A group usually holds the end of one service's run and the start of the next: up to eight runs — or stretches of a run that
            // one list's free candidates cover — in front of the group's first task that is not plain-and-counted are taken this way, one after the other — a run's picks are in the TK row before the
            // next run counts; the lanes behind them are seated and walked as ever, from there.)
            if (prof) wv::keep(cur ^ (u32)inf);   // (the timer below: behind the LDS reads)
            const u64 th1 = prof ? wv::clock64() : 0;
            u32 fdone = 0;   // lanes [0, fdone) have their picks from the run path
            u32 fr_w = 0, fr_b = 0;
            if constexpr (!R7) {
                if (!RING && runs_on && g0 + 64u <= a.block) {   // (the scratch below: 64 pick slots from g0 on)
                    const bool simple = have && plain && !(tflags & 3u);
                    const u64 ns = ~wv::ballot(simple);
                    const u32 nsimple = min(glim, ns ? (u32)wv::ffs64(ns) : 64u);
                    for (u32 it = 0; it < 8u && fdone + 8u <= nsimple; ++it) {
                        const u32 ra = fdone, t_ra = wv::readlane(tmid, ra);
                        const u64 df = wv::ballot(lane >= ra && lane < nsimple && tmid != t_ra);
                        u32 rb = df ? (u32)wv::ffs64(df) : nsimple, rl = rb - ra;
                        if (rl < 8u) break;   // (a short run: the walk is as good)
                        const u32 cur0 = wv::readlane(cur, ra), nent0 = wv::readlane(nent, ra);
                        const u32 k = cur0 + lane;
                        const bool hv = lane < 32u && k < nent0;
                        const u32 hwv = hv ? L_hw[(size_t)k * a.block + g0 + ra] : 0u;
                        const u32 hbv = hv ? L_hb[(size_t)k * a.block + g0 + ra] : 0u;
                        const u32 av = hv ? hbv & ~tk32[hwv] : 0u;
                        const u32 cnt = (u32)wv::popc64((u64)av);
                        const u32 incl = wv::scan_incl_u32(cnt), excl = incl - cnt;
                        const u32 free_ = wv::readlane(incl, 63);
                        if (free_ < rl) {   // lane ra's list holds fewer free candidates than the run has tasks: it serves as many, the next turn
                            if (free_ < 8u) break;   // goes on with the list of the first lane behind them (it starts further into the level)
                            rl = free_;
                            rb = ra + rl;
                        }
                        const u32 ord = wv::mbcnt(wv::ballot(cnt != 0));
                        pk_node[g0 + lane] = 0;   // (scratch: this group's pick slots are written further down, read by its applying wave behind the publish)
                        wv::wave_sync();
                        if (cnt != 0) {
                            if (ra + excl < 64u) pk_node[g0 + ra + excl] = 1;   // a marker at the lane whose rank is the half-word's first
                            pk_idx[g0 + ord] = hwv;
                            pk_idx[g0 + 32u + ord] = av;
                            pk_aux[g0 + ord] = excl;
                        }
                        wv::wave_sync();
                        const u32 upto = wv::scan_incl_u32(pk_node[g0 + lane]);   // half-words that begin at or in front of this lane's rank
                        const bool inr = lane >= ra && lane < rb;
                        const u32 oo = inr ? upto - 1u : 0u;
                        const u32 mav = pk_idx[g0 + 32u + oo], mhw = pk_idx[g0 + oo], rk = inr ? (lane - ra) - pk_aux[g0 + oo] : 0u;
                        u32 bsel = mav;
                        for (u32 t = 0; t < 32u; ++t) {
                            const bool more_ = inr && t < rk;
                            if (!wv::ballot(more_)) break;
                            if (more_) bsel &= bsel - 1u;
                        }
                        if (inr) {
                            fr_w = mhw;
                            fr_b = bsel & (0u - bsel);
                            wv::lds_or32(tk32 + fr_w, fr_b);   // (the next run, the seating and the later groups meet it there)
                        }
                        wv::wave_sync();
                        fdone = rb;
                    }
                }
            }
            const u64 tgb = prof ? wv::clock64() : 0;
            if (prof && g0 >= 128u) late_runs += fdone;   // (reported with the timers)
            if (fdone < glim) seat(plain && lane >= fdone);   // (a second optional step costs more than the stops it saves)
            const u64 tgc = prof ? wv::clock64() : 0;
            if (prof) { cy_g0 += tga - tg0; cy_g1 += tgb - tga; cy_g2 += tgc - tgb; cy_h0 += th0 - tga; cy_h1 += th1 - th0; cy_h2 += tgb - th1; }
            const u64 lanes = glim == 64 ? ~0ull : (1ull << glim) - 1ull;
            const u64 m_plain = wv::ballot(plain), m_inf = wv::ballot(inf), m_exc = wv::ballot(exc), m_unc = wv::ballot(plain && (tflags & 1u));
            // the group ends in front of a task that must use its exception list (its order moves with every placement of the service:
            // only a block's first task may) and behind an uncounted task (its node stays on its level: the later lists are stale about it)
            u32 cut = glim;
            bool last = false;   // the block ends with this group even if the group is walked to its end
            if (m_exc) { cut = (u32)wv::ffs64(m_exc); why = 2; }
            if (m_unc && (u32)wv::ffs64(m_unc) < cut) { cut = (u32)wv::ffs64(m_unc) + 1; why = 3; last = true; }
            {   // tasks with cluster mounts: the block's first one is decided, the block is cut in front of the next (their lists know nothing of each other's volumes)
                const u64 all_csi = wv::ballot(have && (tflags & 2u));
                u64 m_csi = all_csi;
                if (m_csi && !csi_seen) m_csi &= m_csi - 1ull;   // (the first one of the block stays)
                if (m_csi && (u32)wv::ffs64(m_csi) < cut) { cut = (u32)wv::ffs64(m_csi); why = 2; last = false; }
                if (all_csi & (cut >= 64 ? ~0ull : (1ull << cut) - 1ull)) csi_seen = true;
            }
            u32 m_pick = R6_NONE;
            if (g0 == 0 && (m_exc & 1ull)) {   // the block's first task, from its exception list; the block ends behind it
                R6_REACH(R6R_FIRST_EXC, lane == 0);
                if (lane == 0) {
                    pk_node[0] = (u32)exc0_lo + 64u * VW;   // (an address, like the matcher's picks)
                    pk_idx[0] = nc;
                    pk_aux[0] = exc0_entry;
                    if constexpr (R7) {
                        pk_node[0] = r7_addr(m7, sh[8], sh[9]);
                        pk_aux[0] = sh[10];
                    }
                }
                ++nc;
                acc = 1;
                why = 2;
                break;
            }
            // the unrolled walk (wv::match_seq64) passes every lane in order: it serves the plain tasks in front of the cut, the others
            // carry a dummy, and the lane at the cut (if the cut is inside the group) stops it with empty bits
            const bool served = plain && lane < cut;
            if (!served) { bits = lane == cut ? 0u : 1u; bits2 = 0; w = WV_DUMMY_W | lane; }
            u32 pickb = 0, from = fdone;
            u32 flushed = fdone;   // picks of lanes < flushed are in the TK row
            const u64 tg1 = prof ? wv::clock64() : 0;
            if (lane < fdone) { w = fr_w; pickb = fr_b; }   // (the runs' picks are known: the walk starts behind them)
            u64 tw_out = 0;     // (timers: the end of the group's last walk so far; written and read under `prof` only — a copy of a clock value
                                // on the production path is a wait for everything this wave has in flight)
            u32 walks_g = 0;
            [[maybe_unused]] u32 gstops = 0;   // (R6_REACH only)
            R6_REACH(R6R_SHORT_GROUP, lane == 0 && glim < 64u && fdone < cut);
            R6_REACH(R6R_ONE_ENTRY, have && served && win == 1u);
            R6_REACH(R6R_BEHIND_RUNS, lane == 0 && fdone > 0 && fdone < cut);
            R6_REACH(R6R_UNCOUNTED, lane == 0 && m_unc != 0);
            R6_REACH(R6R_MOUNTS, have && (tflags & 2u));
            R6_REACH(R6R_COMPACT, lane == 0 && CPT && VW != 0);
            R6_REACH(R6R_R7, lane == 0 && R7);
            if (fdone < cut) for (;;) {
                const u64 tw_in = prof ? wv::clock64() : 0;
                const u32 at = wv::match_seq64(bits, w, bits2, w2, pickb, lane, from);
                if (prof) {   // (tw_in is first used here, behind the walk: no wait for the clock in front of it)
                    const u64 tw = wv::clock64();
                    cy_s0 += tw - tw_in;
                    if (walks_g) cy_s1 += tw_in - tw_out;
                    tw_out = tw;
                    ++walks;
                    ++walks_g;
                }
                if (at >= cut) break;
                ++reseats;
                R6_REACH(R6R_THREE_STOPS, lane == 0 && ++gstops == 3u);
                R6_REACH(R6R_IDLE_LANES, lane > at && served && !(bits2 == 0 && cur < nent));
                // task `at` ran out of both its half-words — and so, usually, did others that sat on them: this group's picks so far go to
                // the TK row (a pick = the lowest bit the lane had at its turn, in the half-word it still sits on), and every lane still
                // to be served fills its free seats from its cursor on
                if (served && lane >= flushed && lane < at) wv::lds_or32(tk32 + w, pickb & (0u - pickb));
                flushed = at;
                wv::lockstep();   // one wave's LDS operations execute in order: the reads below see the atomics above
                {
                    seat(served && lane >= at);
                    if (wv::readlane(bits, at) == 0) {   // every listed node is taken: propose again against the new state
                        if (prof && lane == at) {   // (off the production path: the list's length from the record itself)
                            const u32 ncd = R7 ? H_meta[li] & 0xFFu : a.prop[li].n_cand;
                            if (ncd >> 31) a.blk->dbg_cut[0] += 1;
                            if (CPT && L_hw[li] < 2u * VW) a.blk->dbg_cut[1] += 1;
                            if ((ncd & 0x7FFFFFFFu) == 1) a.blk->dbg_cut[2] += 1;
                        }
                        cut = at;
                        why = wv::readlane(left_out, at) ? 4 : 1;   // (4: its window ran out, its list had more)
                        if (prof) {   // (a stop no walk follows)
                            const u64 tw = wv::clock64();
                            cy_s1 += tw - tw_out;
                            tw_out = tw;
                        }
                        break;
                    }
                }
                from = at;
            }
            if (prof) { const u64 tg2 = wv::clock64(); cy_load += tg1 - tg0; cy_walk += tg2 - tg1; }
            if (served && lane < cut) m_pick = (w << 5) + (u32)wv::ffs64((u64)pickb);
            if (served && lane >= flushed && lane < cut) wv::lds_or32(tk32 + w, pickb & (0u - pickb));   // for the later groups
            const u64 below = cut == 64 ? ~0ull : (1ull << cut) - 1ull;
            const u64 mc = m_plain & below & lanes, mi = m_inf & below & lanes;
            if (lane < cut && have) {
                if (plain) {
                    pk_node[si] = m_pick;
                    pk_idx[si] = nc + wv::mbcnt(mc);
                    pk_aux[si] = LIST_EMPTY;
                } else {   // no suitable node: final whatever the earlier tasks of the block did (feasibility only shrinks)
                    pk_node[si] = R6_NONE;
                    pk_idx[si] = ni + wv::mbcnt(mi);
                    pk_aux[si] = nc + wv::mbcnt(mc);
                }
            }
            nc += (u32)wv::popc64(mc);
            ni += (u32)wv::popc64(mi);
            acc = g0 + cut;
            if (cut < glim || (last && why == 3)) stop = true;
            else why = 0;
            wv::wave_sync();
            if (lane == 0) wv::lds_publish32(sh + 3, acc);   // the picks of tasks < acc are in the pk arrays: their wave applies them now
            if (prof) cy_s2 += wv::clock64() - (walks_g ? tw_out : tg1);
        }
        if (lane == 0) {
            sh[0] = acc;
            sh[1] = nc;
            sh[2] = ni;
            a.blk->pos = pos + acc;   // (every thread read the old position before the barrier above)
            a.ctl->ncommit = nc;
            a.ctl->ninf = ni;
            wv::lds_publish32(sh + 3, acc);   // (the first task from its exception list leaves the loop before the publish above)
            wv::lds_publish32(sh + 4, 1u);
            a.blk->rounds += 1;
            if (CPT && VW) a.blk->crounds += 1;   // a round with a compact index
            if (why == 1) a.blk->cut_exhausted += 1;
            if (why == 4) a.blk->cut_window += 1;
            if (why == 2) a.blk->cut_exception += 1;
            if (why == 3) a.blk->cut_uncounted += 1;
            a.blk->reseats += reseats;   // (the host's sign of sparse lists: run_blocks switches the compact index on by it)
            if (prof) {
                a.blk->cyc[0] += (u32)((t1 - t0) >> 6);
                a.blk->cyc[1] += (u32)((wv::clock64() - t1) >> 6);
                a.blk->cyc_load += (u32)(cy_load >> 6);
                a.blk->cyc_walk += (u32)(cy_walk >> 6);
                a.blk->cyc_g[0] += (u32)(cy_g0 >> 6);
                a.blk->cyc_g[1] += (u32)(cy_g1 >> 6);
                a.blk->cyc_g[2] += (u32)(cy_g2 >> 6);
                a.blk->cyc_g[3] += seat_steps;
                a.blk->cyc_h[0] += (u32)(cy_h0 >> 6);
                a.blk->cyc_h[1] += (u32)(cy_h1 >> 6);
                a.blk->cyc_h[2] += (u32)(cy_h2 >> 6);
                a.blk->dbg_late_runs += late_runs;
                a.blk->cyc_s[0] += (u32)(cy_s0 >> 6);
                a.blk->cyc_s[1] += (u32)(cy_s1 >> 6);
                a.blk->cyc_s[2] += (u32)(cy_s2 >> 6);
                a.blk->dbg_walks += walks;
            }
            // (tests/emu: a round's outcome, for the comparison of two builds. Flat instances only: a ring's slots hold the picks of the last
            // fifteen groups, not of [0, acc) — its driver checks outcomes, tests/emu/emu_resolve6_ring.cpp)
            if constexpr (!RING) R6_REACH(R6R_ROUND, r6_reach_round(a.blk, pos, acc, why, seat_steps, reseats, pk_node, pk_idx, pk_aux));
        }
    }
    const u64 t2 = prof ? wv::clock64() : 0;
    const u32 base = a.blk->base;
    // NodeInfo.addTask for the accepted pick of block-local task `mine` (record r): the node rows, the bitmaps, the commit log
    auto apply = [&](const u32 mine_task, const u32 mine, const RTask& r) {   // mine: the task's pick slot (== the task but in a ring)
        const u32 t = pos + mine_task, addr = pk_node[mine];
        u32 nd = addr;
        if (CPT) nd = addr == R6_NONE ? R6_NONE : addr < 64u * VW ? a.cidx[addr] : addr - 64u * VW;   // a compact position, or a node behind them
        bool here = true;   // R7: the pick lies in this shard's range
        if constexpr (R7) {
            if (addr != R6_NONE) nd = r7_local(m7, addr, my, &here);
        }
        if (nd == R6_NONE) {   // (every shard records the unplaceable tasks: each explains them over its own nodes)
            a.inf_task[pk_idx[mine]] = t;
            a.inf_pos[pk_idx[mine]] = pk_aux[mine];
        } else if (here) {
            const u32 w = nd >> 6, ci = pk_idx[mine], entry = pk_aux[mine];
            const u64 bit = 1ull << (nd & 63);
            // the node row, requested in one go. No two picks of one block share a node: plain read-modify-write of the row; bitmap
            // words are shared between nodes: atomics
            const i64 qc = a.cpu[nd] - r.cpu, qm = a.mem[nd] - r.mem;
            const u32 old = a.total[nd];
            const int32_t prev = a.last[nd];
            // the node leaves the demand-class rows whose threshold lies in (new residual, old residual]: the rows above the old
            // residual never held it. Thresholds ascend; a batch may have thousands of them, so the upper end is found by bisection.
            if (r.cpu) {
                a.cpu[nd] = qc;
                for (int c = (int)r6_first_above(thr, a.n_dc, qc + r.cpu) - 1; c >= 0 && thr[c] > qc; --c) wv::g_andn64(a.rr + (size_t)c * Wn + w, bit);
            }
            if (r.mem) {
                a.mem[nd] = qm;
                for (int c = (int)r6_first_above(thr + a.n_dc, a.n_dm, qm + r.mem) - 1; c >= 0 && thr[a.n_dc + c] > qm; --c)
                    wv::g_andn64(a.rr + (size_t)(a.n_dc + c) * Wn + w, bit);
            }
            if (r.flags & RT_PORTS)
                for (u32 q = a.pset_off[r.pset]; q < a.pset_off[r.pset + 1]; ++q) wv::g_or64(a.portmap + (size_t)a.pset_ids[q] * Wn + w, bit);
            if (a.n_rg) {   // Claim (resource_management.go:11-72): the count drops by the request; the node leaves the kind's rows it no longer meets
                const u32 gset = a.tg[t];
                for (u32 g = a.gs_off[gset]; g < a.gs_off[gset + 1]; ++g) {
                    const u32 row = a.gs_row[g];
                    int32_t* cp = a.gcnt + (size_t)a.rg_kind[row] * a.gstride + nd;
                    const int32_t c = *cp - a.rg_val[row];
                    *cp = c;
                    for (u32 r2 = a.rg_k0[row]; r2 < a.rg_k1[row]; ++r2)
                        if (a.rg_val[r2] > c) wv::g_andn64(a.rg + (size_t)r2 * Wn + w, bit);
                }
            }
            if (!(r.flags & RT_UNCOUNTED)) {
                a.total[nd] = old + 1;
                const u32 rl = old - base, nl = rl + 1, xm = rl ^ nl;   // the bits a +1 flips: a run of ones from bit 0
                for (u32 b = 0; b < R6_NP && ((xm >> b) & 1u); ++b) wv::g_xor64(a.planes + (size_t)b * Wn + w, bit);
                wv::g_max32(&a.blk->maxrel, nl);
                if (nl >> R6_NP) a.blk->error = ERR_LEVEL_RANGE;
                if (entry == LIST_EMPTY) {
                    wv::g_or64(a.X + (size_t)r.svc * a.xs + w, bit);
                    a.list_node[r.slot] = nd;
                    a.list_svc[r.slot] = 1;
                    a.list_fail[r.slot] = 0;
                } else
                    a.list_svc[entry] += 1;
            }
            a.log_node[ci] = nd;
            a.log_task[ci] = t;
            a.log_prev[ci] = prev;
            a.last[nd] = (int32_t)ci;
            a.out_node[t] = (int32_t)nd;
            if (CSI && a.csi_of) {   // chooseTaskVolumes + reserveTaskVolumes on the node (scheduler.go:857-874); a mount without a volume: assigned without attachments
                const u32 ck = a.csi_of[t];
                if (ck != R6_NONE) {
                    u32 att[VOL_MAX_MOUNTS];
                    const u32 set = a.csi_set[ck], na = vol_choose(a.vol, set, nd, att, nullptr);
                    if (na) vol_reserve(a.vol, set, nd, att, na);
                    for (u32 q = 0; q < VOL_MAX_MOUNTS; ++q) a.att[(size_t)ck * VOL_MAX_MOUNTS + q] = att[q];
                    if constexpr (R7) {
                        if (na) r7_leave_trailer(a, my, rnd, set, nd, att, na);   // the other shards reserve the same volumes at the start of the next round
                    }
                }
            }
        }
    };
    if constexpr (R7) {
        // a wave waits (polling LDS, asleep in between) until its group is matched or the matching is over, and applies what was accepted of it
        if (wave_ != 0) {
            const u32 g0 = (wave_ - 1u) * 64u, need = min(g0 + 64u, n);
            if (g0 > 0 && g0 < n)
                while (wv::lds_poll32(staged + (g0 >> 6)) == 0) wv::spin_pause();
            if (g0 > 0 && mine0 < n) {
                // until the matcher reaches this wave's group: move every task's cursor over the entries that are dead by now (taken nodes
                // stay taken: what is dead against an older TK row is dead), so that the matcher seats the group in a step or two
                const u32 lv = H_level[mine0], nent = lv != R6_NONE ? (H_meta[mine0] & 0xFFu) : 0u;
                const u32* tk32 = reinterpret_cast<const u32*>(tk);
                u32 cur = 0;
                while (wv::lds_poll32(sh + 3) + 64u < g0 && wv::lds_poll32(sh + 4) == 0) {   // (stops a group early: the last value must be in LDS when it is read)
                    for (int q = 0; q < 4 && cur < nent; ++q) {
                        if (L_hb[(size_t)cur * a.block + mine0] & ~tk32[L_hw[(size_t)cur * a.block + mine0]]) break;
                        ++cur;
                    }
                    L_cur[mine0] = cur;
                    wv::spin_pause();
                }
            }
            if (g0 < n)
                while (wv::lds_poll32(sh + 3) < need && wv::lds_poll32(sh + 4) == 0) wv::spin_pause();
        }
        const u32 acc_now = wv::readfirstlane(wv::lds_poll32(sh + 3));
        if (mine0 < acc_now) apply(mine0, mine0, r0);
    } else if (wave_ != 0) {
        // Helper h = wave - 1 takes the groups h, h + 15, ... in order: it stages the group's windows (g >= 2), moves the cursors over
        // entries that die while the matcher works on the group before, waits for the group's picks and applies them. Every wait polls
        // a word only wave 0 advances (sh[3]: tasks decided so far) and leaves when the matching is over (sh[4], read FIRST: sh[3] is
        // final then); a helper that finds its group undecided at the end is done, the groups behind it are undecided as well.
        const u32* tk32 = reinterpret_cast<const u32*>(tk);
        RTask r = r0;
        for (u32 g = wave_ - 1u; g * 64u < n; g += 15u) {
            const u32 g0 = g * 64u, j = g0 + lane, need = min(g0 + 64u, n);
            const u32 sj = RING ? g0 % RS + lane : j;   // the task's slot
            const bool have = j < n;
            u32 cnt = 0, left = 0, hbits = 0;   // hbits: the head's bits of the task's L_cur word
            if (g >= 2u) {
                const u32 jj = have ? j : 0u;
                const R6Prop* q = a.prop + jj;
                using Ext = typename std::conditional<RING, R6PropExtRing, R6PropExt>::type;   // (a ring round's records: written by the _r propose instances)
                const Ext* x = a.ext ? reinterpret_cast<const Ext*>(a.ext) + jj : nullptr;
                const u32 lv = q->level, nc = q->n_cand;
                hbits = r6_head_bits(lv, q->exc_hi, q->flags);
                if (runs_on && have) pk_idx[sj] = a.tmpl[pos + j];   // (this wave applied the group fifteen in front of this one before it came here: other slots)
                const u32 total = (have && lv != R6_NONE) ? (nc & 0x7FFFFFFFu) : 0u;   // (beyond 2 * R6_CAND only with an extension)
                u32 at = 0;   // the entries in front of it are dead (whole batches of sixteen)
                // The window from the TK row as it is: sixteen entries of the list at a time through registers, from `at` on, the live ones
                // into the task's slot until it is full. `left`: the list goes on behind what was looked at, or behind the window.
                auto stage = [&]() {
                    cnt = 0;
                    left = total ? nc >> 31 : 0u;
                    bool lead = true;
                    u32 p = at;
                    while (p < total && cnt < win) {
                        const u32* ph = p < 2u * R6_CAND ? reinterpret_cast<const u32*>(q->hw) + p / 2u : reinterpret_cast<const u32*>(x->hw) + (p - 2u * R6_CAND) / 2u;
                        const u32* pb = p < 2u * R6_CAND ? q->hb + p : x->hb + (p - 2u * R6_CAND);
                        u32 hwv[16], hbv[16], tkv[16];
                        WV_UNROLL
                        for (int k = 0; k < 8; ++k) {
                            const u32 v = ph[k];
                            hwv[2 * k] = v & 0xFFFFu;
                            hwv[2 * k + 1] = v >> 16;
                        }
                        WV_UNROLL
                        for (int k = 0; k < 16; ++k) hbv[k] = pb[k];
                        WV_UNROLL
                        for (int k = 0; k < 16; ++k) tkv[k] = tk32[p + (u32)k < total ? hwv[k] : 0u];   // (what lies behind the list's end is not an index)
                        bool any = false;
                        WV_UNROLL
                        for (int k = 0; k < 16; ++k)
                            if (p + (u32)k < total && (hbv[k] & ~tkv[k])) {
                                any = true;
                                if (cnt < win) {
                                    L_hw[(size_t)cnt * RS + sj] = (unsigned short)hwv[k];
                                    L_hb[(size_t)cnt * RS + sj] = hbv[k];
                                    ++cnt;
                                } else
                                    left = 1;
                            }
                        p += 16u;
                        if (lead && !any && p < total) at = p;
                        else lead = false;
                    }
                    if (p < total) left = 1;
                    if (have) {
                        for (u32 k = cnt; k < win; ++k) L_hw[(size_t)k * RS + sj] = 0;   // (as the prologue's: a valid TK word behind every entry the seating step may read)
                        L_cur[sj] = (cnt << 8) | (left << 16) | hbits;
                    }
                    if constexpr (RING) {
                        R6_RING_REACH(R6RR_SKIPPED3, have && at >= 48u);
                        R6_RING_REACH(R6RR_WRAPPED_STAGE, lane == 0 && g >= 15u);
                    }
                };
                // Taken nodes stay taken, so a window staged against an older TK row holds nothing wrong, only entries that may have died
                // since (the cursor loop and the seating step meet those): the slot is staged again whenever the matcher publishes a group,
                // loads and all, while there is time — when the picks of group g - 2 are out it is ready but for that group's picks, and is
                // published at once: no load between the matcher and the group. (A helper that comes late stages then.)
                // Only the helpers of the next few groups do so: the uncoalesced loads of many waves queue up in the CU's one address path,
                // in front of the matcher's own (all helpers at once at the kernel's start: 15 k cycles of every round's prologue).
                // (Windows of 2 * R6_CAND rows — batches of runs, whose groups the matcher is through in a few thousand cycles: nothing to
                // wait for, a window is the front of the list. Staged right away, two groups at a time in group order as the prologue's —
                // the one wait in this kernel on a word a HELPER advances (staged[g - 2]): staging there depends on nothing the matcher
                // does, so the chain g - 2, g - 4, ... ends at the prologue's two groups; it leaves on sh[4] like every other.)
                u32 seen = 0;
                bool fresh = false;
                if (LW == LMAX) {
                    for (;;) {
                        const bool over = wv::lds_poll32(sh + 4) != 0;
                        if (wv::lds_poll32(staged + (g - 2u)) != 0 || over) break;
                        wv::spin_pause();
                    }
                    stage();
                    fresh = true;
                }
                for (;;) {
                    const bool over = wv::lds_poll32(sh + 4) != 0;
                    const u32 acc = wv::lds_poll32(sh + 3);
                    if (acc + 64u >= g0 || over || LW == LMAX) break;
                    if (acc != seen && acc + 192u >= g0) {
                        seen = acc;
                        stage();
                        fresh = true;
                    }
                    wv::spin_pause();
                }
                if (LW != LMAX && wv::lds_poll32(sh + 3) + 64u < g0) break;   // (over: the block was cut in front of group g - 1)
                if (!fresh) stage();
                wv::lockstep();
                if (lane == 0) wv::lds_publish32(staged + g, 1u);
            }
            if (g >= 15u && have) r = a.rt[pos + j];   // (the first group's record was requested in the prologue)
            u32 cur = 0;
            for (;;) {
                const bool over = wv::lds_poll32(sh + 4) != 0;
                const u32 acc = wv::lds_poll32(sh + 3);
                if (acc >= need || over) break;
                if (g >= 2u && have && acc < g0) {   // (the matcher reads the cursor when it starts on the group; a later value is lost, no harm)
                    for (int q = 0; q < 4 && cur < cnt; ++q) {
                        if (L_hb[(size_t)cur * RS + sj] & ~tk32[L_hw[(size_t)cur * RS + sj]]) break;
                        ++cur;
                    }
                    L_cur[sj] = cur | (cnt << 8) | (left << 16) | hbits;
                }
                wv::spin_pause();
            }
            const u32 acc_now = wv::readfirstlane(wv::lds_poll32(sh + 3));
            if (j < acc_now) apply(j, sj, r);
            if (acc_now < need) break;
        }
    }
    if (prof && wave_ == 1 && lane == 0) a.blk->cyc[3] += (u32)((wv::clock64() - t2) >> 6);   // the first group's applying wave: waiting for it + applying
    if constexpr (CPT && !R7) {
        if (a.compact == 2u) {   // the next round's compact index, here instead of in a launch of its own (r6_compact_body)
            wv::wait_vm();       // this wave's atomics on the rows have arrived ...
            wv::barrier();       // ... and every other wave's; nobody reads the TK row any more (the body's 32 words lie on it)
            const u32 np = pos + sh[0];
            const bool go = np < end && wv::readfirstlane(wv::g_fresh32(&a.blk->error)) == ERR_NONE;
            wv::barrier();       // (sh[0] is read before the body's first barrier lets anybody write LDS)
            if (go) r6_compact_body<true>(a, np, reinterpret_cast<u32*>(wv::lds()));
        }
    }
}
WV_KERNEL(R6_COMMIT_THREADS) void k_r6_commit(R6Args a) { r6_commit_t<false, false>(a); }
WV_KERNEL(R6_COMMIT_THREADS) void k_r6_commit_c(R6Args a) { r6_commit_t<true, false>(a); }   // ... with a compact index (launched behind k_r6_compact only)
WV_KERNEL(R6_COMMIT_THREADS) void k_r6_commit_v(R6Args a) { r6_commit_t<false, true>(a); }   // ... for a batch with cluster mounts (R6Args.csi_of)
#if R6_RING_ON
WV_KERNEL(R6_COMMIT_THREADS) void k_r6_commit_r(R6Args a) { r6_commit_t<false, false, false, true>(a); }   // ... a ring round (R6Args.ring != 0): blocks beyond the LDS
#endif

#endif   // SWP_R6_KERNELS

}  // namespace swpdev
