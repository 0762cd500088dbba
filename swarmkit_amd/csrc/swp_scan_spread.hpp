// swp_scan_spread.hpp — the SPREAD instance of the scan resolver: one-off tasks whose Placement.Preferences create spread levels, decided
// inside a batch, one after the other, by ALL threads of one workgroup over ALL nodes (k_scan with one more reduction dimension).
//
// What the reference does for such a task (a group of ONE: scheduler.go:696-748): nodeSet.tree with maxAssignments = 1 (nodeset.go:50-124)
// — every node of the nodeSet adds its ActiveTasksCountByService to every branch on its path, whether it passes the filters or not
// (:88-90, :103-105), and every leaf's heap of one ends up with the leaf's least node by nodeLess among those that pass, the FIRST one
// in node order among equals (:115 is strict; the canonical node order is the index order) — and then scheduleNTasksOnSubtree
// (scheduler.go:772-825) with n = 1 at the root. With one task in the group the first leaf that holds a node takes it
// (scheduleNTasksOnNodes places it on nodes[0] and the group map is empty: whatever the walk does afterwards changes nothing), so the walk
// is run literally up to that leaf: desired / remainder / noRoom / tasksInUsableBranches per frame, the children in creation order
// (tn_first / tn_next: first seen in node order), a child called with the tasksToAssign its parent computed (which may be more than one:
// the branch that is handed five tasks spreads five over ITS children). A task without preferences is a tree of one node, the same path.
//
// Per task: every thread evaluates its nodes by k_scan's filter lines and k_scan's packed key (hi << 32 | total << 12 | node) and puts a
// feasible node's key into leafmin[leaf of the node] (LDS min) and every present node's count of the service into tsum[leaf] (LDS add);
// barrier; wave 0 adds the sums up the tree (a level at a time, deepest first) and its first lane walks; barrier; the owner of the
// picked node applies NodeInfo.addTask exactly as k_scan does. The per-tree words (leafmin, tsum, noroom) exist twice and alternate
// between tasks: the set of the NEXT task is cleared in front of this task's first barrier (its last reader, the walk two tasks ago,
// ended in front of that task's second barrier). An unplaced task goes to inf_task / inf_pos: nothing passed in any leaf, so tree()
// called the pipeline on every node of the nodeSet once — the batch's Explain pass is the plain first-fail histogram, unchanged.
//
// Written against swp_wave.hpp only (tests/emu/emu_scan_spread.cpp runs it on CPU fibers against a sequential model).
#pragma once
#include <type_traits>

#include "swp_scan.hpp"

namespace swpdev {

#define ERR_SPREAD_WALK 4   // the walk of a task exceeded its bound of passes (it converges: a bug, or tables that are no tree): the launch goes on, the batch fails

struct SpreadArgs {
    ScanArgs s;             // the stretch [j0, j1), the (service, node) matrices of k_scan_fill / k_scan_lists over all nodes
    const u32* ttree;       // [tasks of the batch] the task's tree (a task without preferences: the tree of no levels)
    const u32* tree_off;    // [trees + 1] first tree node of a tree; the tables below are indexed by tree_off[tree] + local index, local 0 = the root
    const u32* tn_parent;   // local index of the parent (the root: 0xFFFFFFFF); a child follows its parent in the table
    const u32* tn_first;    // first child in creation order, 0xFFFFFFFF: a leaf
    const u32* tn_next;     // next sibling in creation order
    const u32* tn_nchild;   // len(tree.next)
    const u32* tn_depth;    // levels above the tree node (the root: 0)
    const u32* leaf_of_node;   // [trees][n_nodes] local index of the node's leaf, 0xFFFFFFFF: the node is not in the nodeSet
    u32 max_ntn, max_depth; // over the batch's trees: tree nodes of the largest, levels of the deepest
    u32 n_trees, tot_ntn;   // trees; tree nodes of all of them (tree_off[n_trees]): the tables' length — the kernel keeps them in LDS
    // the compact instance (k_scan_spread<.., true>, below) only; null / 0 for the plain one
    const u32* tpair;       // [tasks of the batch] the task's (service, tree) pair
    const u32* base;        // [n_pairs][max_ntn] a pair's leaf sums over the nodes OUTSIDE the segment's union (k_spread_base)
    u32 n_pairs;
};

struct SpFrame {   // one invocation of scheduleNTasksOnSubtree that went past the leaf test (scheduler.go:784-822)
    i64 usable, desired, rem;   // tasksInUsableBranches, desiredTasksPerBranch, remainder
    u32 tn, child, n_noroom, converging;
};
// node rows + the result word + two sets of (leafmin, tsum, noroom) per tree node of the largest tree + a frame per level + the trees'
// tables (tree_off and the five per-tree-node words: the walk is a chain of dependent reads, a global round trip each otherwise)
inline __host__ __device__ size_t scan_lds_sp(u32 n_nodes, u32 max_ntn, u32 max_depth, u32 n_trees, u32 tot_ntn) {
    return (((size_t)n_nodes * 24 + 15) & ~(size_t)15) + 16 + (size_t)2 * max_ntn * 16 + (size_t)(max_depth + 1) * sizeof(SpFrame) + ((size_t)n_trees + 1 + (size_t)5 * tot_ntn) * 4;
}

// ---- a compact spread segment whose union is too wide for the kernel above: k_spread_cut finds where to CUT it
// The rule, over the static class rows row(t) = sc[rt[t].sc] of the segment's tasks [j0, j1) and a limit of L nodes:
//   a piece starts at a task with preferences (j0 is one) and takes the tasks behind it while the union of their rows stays at or
//   below L nodes; in front of the first task k that does not fit the piece ends. If k has preferences the next piece starts at it;
//   else the tasks from k up to the next task with preferences (or j1) form a PLAIN piece — the block / scan resolver's — and the next
//   piece starts behind it. A piece's first task whose own row exceeds L cannot be taken at all: CUT_OWN_ROW.
// Cutting is exact wherever it happens (swp_rounds.hpp spread_segments): consecutive pieces decide the tasks in array order.
#define CUT_OK 0u
#define CUT_OWN_ROW 1u      // out[1]: the task
#define CUT_FULL 2u         // more than max_pieces pieces
#define CUT_HEAD 4u         // words in front of the piece list
struct CutArgs {
    const RTask* rt;        // the batch's tasks (rt[].sc: the static class row)
    const u32* pref;        // [tasks of the batch] != 0: the task has preferences
    const u64* sc;          // [n_sc][n_words] the static class rows
    u64* cu;                // [n_words] the piece's union when it does not fit in LDS (u_lds == 0)
    u32* out;               // [CUT_HEAD + 3 * max_pieces]: status, task, pieces, counts made; then (first, count, spread) per piece
    u32 j0, j1, n_sc, n_words, L, max_pieces, u_lds;
};
// a mask and a sum per wave, a chunk's class rows and preference words, a flag per class row, the union's words
inline __host__ __device__ size_t spread_cut_lds(u32 n_sc, u32 n_words, bool u_lds) {
    return (size_t)(SCAN_THREADS / 64) * 12 + (size_t)2 * SCAN_THREADS * 4 + (((size_t)n_sc * 4 + 7) & ~(size_t)7) + (u_lds ? (size_t)n_words * 8 : 0);
}

#ifdef SWP_SCAN_SPREAD_KERNEL
// ONE workgroup. The tasks are taken SCAN_THREADS at a time, a task a thread: its class row and preference word go to LDS once, and
// a flag per class row says whether the piece holds the row already. A ballot of the tasks whose row it does not hold yet finds the
// next task that costs anything; the tasks in front of it join the piece unseen. That task costs ONE count: every thread takes the
// words w = tid, tid + SCAN_THREADS, ... of popc(U | row), a DPP reduction per wave, a word per wave in LDS. A thread reads and writes
// only ITS words of U (in LDS or, beyond it, in cu), so U needs no barrier of its own. Every branch below is uniform over the
// workgroup: what it tests was read from LDS behind a barrier.
//   barrier A: the waves' masks are written;  barrier B: the waves' sums are written (and the masks read);  barrier C: a chunk's words
//   are written (and everything of the chunk in front read). A flag is written in front of A or B and read behind C.
WV_KERNEL(SCAN_THREADS) void k_spread_cut(CutArgs p) {
    constexpr u32 NW = SCAN_THREADS / 64;
    const u32 tid = wv::tid(), lane = wv::lane(), wave = tid >> 6, Wn = p.n_words;
    u64* wmask = wv::lds();                                  // [NW] a wave's tasks that still cost a count (or: that have preferences)
    u32* wsum = reinterpret_cast<u32*>(wmask + NW);          // [NW] a wave's share of a count
    u32* tsc = wsum + NW;                                    // [SCAN_THREADS] the chunk's class rows
    u32* tpf = tsc + SCAN_THREADS;                           // [SCAN_THREADS] ... and preference words
    u32* flag = tpf + SCAN_THREADS;                          // [n_sc] the piece holds the row
    u64* U = p.u_lds ? reinterpret_cast<u64*>(flag + ((p.n_sc + 1u) & ~1u)) : p.cu;
    for (u32 w = tid; w < Wn; w += SCAN_THREADS) U[w] = 0;
    for (u32 c = tid; c < p.n_sc; c += SCAN_THREADS) flag[c] = 0;
    u32 j = p.j0, np = 0, counts = 0, status = CUT_OK, bad = 0, skip0 = 0;
    bool fresh = true, skipping = false;   // fresh: the piece holds no row yet; skipping: inside a plain piece, looking for its end
    auto emit = [&](u32 first, u32 n, u32 spread) {
        if (np == p.max_pieces) { status = CUT_FULL; return; }
        if (tid == 0) { p.out[CUT_HEAD + 3 * np] = first; p.out[CUT_HEAD + 3 * np + 1] = n; p.out[CUT_HEAD + 3 * np + 2] = spread; }
        ++np;
    };
    for (u32 c0 = p.j0; c0 < p.j1 && status == CUT_OK; c0 += SCAN_THREADS) {
        const u32 cend = p.j1 - c0 < SCAN_THREADS ? p.j1 - c0 : SCAN_THREADS;
        const bool have = tid < cend;
        const u32 my_sc = have ? p.rt[c0 + tid].sc : 0u, my_pf = have ? p.pref[c0 + tid] : 0u;
        tsc[tid] = my_sc;
        tpf[tid] = my_pf;
        wv::barrier();   // C
        bool need = have && !flag[my_sc];
        u32 cur = 0;   // the chunk's tasks in front of it are decided
        while (cur < cend && status == CUT_OK) {
            const u64 m = wv::ballot(tid >= cur && (skipping ? have && my_pf != 0 : need));
            if (lane == 0) wmask[wave] = m;
            wv::barrier();   // A
            u32 i = cend;
            for (u32 v = 0; v < NW; ++v) {
                const u64 x = wmask[v];
                if (x) { i = v * 64u + (u32)wv::ffs64(x); break; }
            }
            if (i == cend) break;   // the rest of the chunk rides along (the next write of wmask lies behind C)
            if (skipping) {   // the plain piece ends in front of this task with preferences: the next piece starts at it
                emit(skip0, c0 + i - skip0, 0u);
                skipping = false;
                j = c0 + i;
                cur = i;
                wv::barrier();   // (the masks are read: no B on this path)
                continue;
            }
            const u32 r = tsc[i];
            const u64* row = p.sc + (size_t)r * Wn;
            u32 part = 0;
            for (u32 w = tid; w < Wn; w += SCAN_THREADS) part += (u32)wv::popc64(U[w] | row[w]);
            const u32 incl = wv::scan_incl_u32(part);
            if (lane == 63) wsum[wave] = incl;
            wv::barrier();   // B
            u32 total = 0;
            for (u32 v = 0; v < NW; ++v) total += wsum[v];
            ++counts;
            if (total <= p.L) {   // the task joins the piece, and with it every task of the same row
                for (u32 w = tid; w < Wn; w += SCAN_THREADS) U[w] |= row[w];
                if (tid == 0) flag[r] = 1u;
                if (my_sc == r) need = false;
                fresh = false;
                cur = i + 1u;
            } else if (fresh) {   // its own row is too wide
                status = CUT_OWN_ROW;
                bad = c0 + i;
            } else {   // the cut: the piece ends in front of the task, which is looked at again with nothing in U
                emit(j, c0 + i - j, 1u);
                for (u32 w = tid; w < Wn; w += SCAN_THREADS) U[w] = 0;
                for (u32 c = tid; c < p.n_sc; c += SCAN_THREADS) flag[c] = 0;
                fresh = true;
                need = have;
                cur = i;
                if (tpf[i]) j = c0 + i;
                else { skipping = true; skip0 = c0 + i; }
            }
        }
    }
    if (status == CUT_OK) {
        if (skipping) emit(skip0, p.j1 - skip0, 0u);
        else emit(j, p.j1 - j, 1u);
    }
    if (tid == 0) { p.out[0] = status; p.out[1] = bad; p.out[2] = np; p.out[3] = counts; }
}

// The compact instance's base sums. nodeSet.tree adds a node's count of the service to every branch on its path whether the node passes
// the filters or not, so a node outside the segment's union — never picked, never changed inside the segment — still weighs on the
// walk: with a constant, per (service, tree) pair. base[pair][leaf] = the sum of list_svc over the service's list entries whose node lies
// outside the union (cu bit clear) and has a leaf in the pair's tree. base zeroed before; grid (list entries / 256, pairs), as
// k_scan_lists_c; from the lists as they are when the segment begins. A pair of tree 0 (one leaf: its sum is never read) is left at 0.
// (many workgroups add to a pair's row. On the CPU fibers one thread runs at a time: a plain add, as r6_count32)
#if defined(__HIPCC__)
WV_DEV void sp_add32(u32* p, u32 v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#else
inline void sp_add32(u32* p, u32 v) { *p += v; }
#endif
WV_KERNEL(256) void k_spread_base(SpreadArgs p, const u32* pair_svc, const u32* pair_tree, u32* base) {
    const u32 pr = wv::block_y(), svc = pair_svc[pr], tree = pair_tree[pr];
    if (tree == 0) return;
    const ScanArgs& s = p.s;
    const u32 ntn = p.tree_off[tree + 1] - p.tree_off[tree];
    const u32 e0 = s.a.list_off[svc], e1 = s.a.list_off[svc + 1];
    for (u32 e = e0 + wv::block() * 256 + wv::tid(); e < e1; e += 256u * 64u) {
        const u32 n = s.a.list_node[e];
        if (n == LIST_EMPTY || ((s.cu[n >> 6] >> (n & 63)) & 1ull)) continue;   // (inside the union: the kernel adds it, task by task)
        const u32 lf = p.leaf_of_node[(size_t)tree * s.a.n_nodes + n], sv = s.a.list_svc[e];
        if (lf >= ntn || sv == 0) continue;   // (0xFFFFFFFF: the node is not in the nodeSet)
        sp_add32(base + (size_t)pr * p.max_ntn + lf, sv);
    }
}

// scheduleNTasksOnSubtree with one task, up to the first leaf that holds a node: its key (KEY_NONE: no leaf does). One thread.
// tn_first / tn_next / tn_nchild: the tree's own rows of the tables (local indices); max_depth: the frames there are
WV_DEV u64 spread_walk(const u32* tn_first, const u32* tn_next, const u32* tn_nchild, u32 max_depth, u32 ntn, const u64* leafmin, const u32* tsum, u32* noroom, SpFrame* st, bool* hang) {
    if (tn_first[0] == LIST_EMPTY) return leafmin[0];   // the tree is one leaf
    int sp = 0;
    u32 passes = 0;
    st[0].tn = 0;
    st[0].usable = tsum[0];
    st[0].n_noroom = 0;
    st[0].converging = 1;
    st[0].child = LIST_EMPTY;
    // tasksScheduled is 0 in every frame until a leaf takes the task, and then the walk is over: `remainder` never drops, and a frame's n
    // — the tasksToAssign of the call that made it — can be computed again from the caller's frame whenever the frame needs it
    bool fresh = true;   // the frame on top starts a pass of its while loop
    while (sp >= 0) {
        SpFrame& f = st[sp];
        const u32 nch = tn_nchild[f.tn];
        if (fresh) {   // `for tasksScheduled != n && len(noRoom) != len(tree.next) && converging`
            i64 n = 1;
            if (sp > 0) {
                const SpFrame& up = st[sp - 1];
                n = up.desired - (i64)tsum[f.tn] + (up.rem > 0 ? 1 : 0);
            }
            const i64 room = (i64)nch - (i64)f.n_noroom;
            if (room == 0 || !f.converging) {   // returns 0: the caller notes noRoom
                --sp;
                if (sp >= 0) {
                    SpFrame& up = st[sp];
                    noroom[up.child] = 1;
                    up.n_noroom++;
                    up.usable -= (i64)tsum[up.child];
                    up.child = tn_next[up.child];
                    fresh = false;
                }
                continue;
            }
            if (++passes > 2u * ntn) { *hang = true; return KEY_NONE; }
            const i64 tot = f.usable + n;
            f.desired = tot / room;
            f.rem = tot % room;
            f.converging = 0;
            f.child = tn_first[f.tn];
            fresh = false;
        }
        // `for _, subtree := range tree.next` in creation order, from f.child on
        bool called = false;
        while (f.child != LIST_EMPTY) {
            const u32 c = f.child;
            if (!noroom[c]) {
                const i64 sub = tsum[c];
                if (sub < f.desired || (sub == f.desired && f.rem > 0)) {
                    f.converging = 1;
                    if (tn_first[c] == LIST_EMPTY) {   // a leaf: it takes the task iff its heap holds a node
                        if (leafmin[c] != KEY_NONE) return leafmin[c];
                        noroom[c] = 1;   // res = 0 < tasksToAssign
                        f.n_noroom++;
                        f.usable -= sub;
                    } else {
                        if ((u32)sp + 1u > max_depth) { *hang = true; return KEY_NONE; }   // (a frame per level: deeper than the tables say)
                        SpFrame& d = st[sp + 1];
                        d.tn = c;
                        d.usable = sub;
                        d.n_noroom = 0;
                        d.converging = 1;
                        d.child = LIST_EMPTY;
                        ++sp;
                        fresh = true;
                        called = true;
                        break;
                    }
                }
            }
            f.child = tn_next[c];
        }
        if (!called) fresh = true;   // the range is through: the while condition again
    }
    return KEY_NONE;
}

// SCAN_CM: the COMPACT instance (a nodeSet beyond SCAN_MAXN slots, a segment whose class rows' union is not; swp_scan.hpp) — N is the
// union's node count, the LDS rows, the matrices and the key's low 12 bits carry the compact index c (cmap ascending: the lowest c among
// equal keys is the lowest node), everything that is indexed by node in global memory or leaves the kernel the node behind it (`real`, in
// registers for the segment), and a task's leaf sums start from its pair's base row (k_spread_base) instead of 0. false: the plain code.
template <int SCAN_NQ, bool SCAN_CM = false>
WV_KERNEL(SCAN_THREADS) void k_scan_spread(SpreadArgs p) {
    const ScanArgs& s = p.s;
    const R6Args& a = s.a;
    const u32 tid = wv::tid(), lane = wv::lane(), N = SCAN_CM ? s.n_c : a.n_nodes, Wn = a.n_words, M = p.max_ntn;
    unsigned char* l = reinterpret_cast<unsigned char*>(wv::lds());
    i64* cpu = reinterpret_cast<i64*>(l);
    i64* mem = cpu + N;
    u32* tot = reinterpret_cast<u32*>(mem + N);
    int32_t* lastc = reinterpret_cast<int32_t*>(tot + N);
    u64* res = reinterpret_cast<u64*>(l + (((size_t)N * 24 + 15) & ~(size_t)15));   // [2] the walk's answer, alternating
    u64* lmin = res + 2;                                   // [2][M] a leaf's least key
    u32* lsum = reinterpret_cast<u32*>(lmin + 2 * (size_t)M);   // [2][M] tree.tasks
    u32* lnor = lsum + 2 * (size_t)M;                      // [2][M] noRoom
    SpFrame* frames = reinterpret_cast<SpFrame*>(lnor + 2 * (size_t)M);   // [max_depth + 1]
    u32* l_off = reinterpret_cast<u32*>(frames + p.max_depth + 1);       // [n_trees + 1] tree_off
    u32* l_parent = l_off + p.n_trees + 1;                                // [tot_ntn] each: the trees' tables
    u32* l_first = l_parent + p.tot_ntn;
    u32* l_next = l_first + p.tot_ntn;
    u32* l_nchild = l_next + p.tot_ntn;
    u32* l_depth = l_nchild + p.tot_ntn;
    if (a.blk->error != ERR_NONE) return;
    const u32 first = s.j0 < s.j1 ? s.j0 : 0u, last = s.j0 < s.j1 ? s.j1 - 1u : 0u;   // (reads beyond the stretch are clamped to its last task and never used)
    const u32 second = s.j0 + 1u < s.j1 ? s.j0 + 1u : last;
    u32 real[SCAN_NQ];   // SCAN_CM: the nodes behind this thread's rows, fixed for the segment
    if (!SCAN_CM) {
        for (u32 n = tid; n < N; n += SCAN_THREADS) { cpu[n] = a.cpu[n]; mem[n] = a.mem[n]; tot[n] = a.total[n]; lastc[n] = a.last[n]; }
        for (u32 i = tid; i < 2 * M; i += SCAN_THREADS) { lmin[i] = KEY_NONE; lsum[i] = 0; lnor[i] = 0; }
    } else {
        WV_UNROLL
        for (int q = 0; q < SCAN_NQ; ++q) {
            const u32 n = tid + (u32)q * SCAN_THREADS, m = n < N ? s.cmap[n] : 0u;
            real[q] = m;
            if (n < N) { cpu[n] = a.cpu[m]; mem[n] = a.mem[m]; tot[n] = a.total[m]; lastc[n] = a.last[m]; }
        }
        const u32* b0 = p.base + (size_t)p.tpair[first] * M;   // the first task's set starts from its pair's base sums
        for (u32 i = tid; i < 2 * M; i += SCAN_THREADS) { lmin[i] = KEY_NONE; lsum[i] = i < M ? b0[i] : 0u; lnor[i] = 0; }
    }
    for (u32 i = tid; i <= p.n_trees; i += SCAN_THREADS) l_off[i] = p.tree_off[i];
    for (u32 i = tid; i < p.tot_ntn; i += SCAN_THREADS) {
        l_parent[i] = p.tn_parent[i]; l_first[i] = p.tn_first[i]; l_next[i] = p.tn_next[i]; l_nchild[i] = p.tn_nchild[i]; l_depth[i] = p.tn_depth[i];
    }
    u32 present = 0;   // bit q: this thread's q-th node is in the nodeSet
    WV_UNROLL
    for (int q = 0; q < SCAN_NQ; ++q) {
        const u32 n = tid + (u32)q * SCAN_THREADS, m = SCAN_CM ? real[q] : n;
        if (n < N && ((a.valid[m >> 6] >> (m & 63)) & 1ull)) present |= 1u << q;
    }
    u32 nc = a.ctl->ncommit, ni = a.ctl->ninf;
    // What a task reads from global memory is requested AHEAD, as k_scan does: the three words that say where the rest lies — its
    // class row, its service, its tree — two tasks ahead (the record's cache line comes with them); what hangs on those three — the static-class word, the key
    // half, the list entry and the leaf of each of this thread's nodes — one task ahead. A task's turn then starts with everything in
    // registers. The one value the task in between can change, the key half (and the entry) of the node it takes, is corrected by
    // that node's owner.
    u32 sc_n = a.rt[first].sc, svc_n = a.rt[first].svc, tree_n = p.ttree[first];
    u32 sc_nn = a.rt[second].sc, svc_nn = a.rt[second].svc, tree_nn = p.ttree[second];
    // (SCAN_CM, four nodes a thread: the register file is the limit — the class word is kept as the 32-bit half that holds the node's bit)
    typename std::conditional<SCAN_CM, u32, u64>::type scn[SCAN_NQ];
    u32 hin[SCAN_NQ], ein[SCAN_NQ], lfn[SCAN_NQ];
    const u32* sc32 = reinterpret_cast<const u32*>(a.sc);
    auto ahead = [&](u32 sc_, u32 svc_, u32 tree_) {   // this thread's nodes for the task with this class row, service and tree
        WV_UNROLL
        for (int q = 0; q < SCAN_NQ; ++q) {
            const u32 n = tid + (u32)q * SCAN_THREADS, m = SCAN_CM ? real[q] : n;
            const bool in = (present >> q) & 1u;
            if (SCAN_CM) scn[q] = in ? sc32[(size_t)sc_ * Wn * 2u + (m >> 5)] : 0u;
            else scn[q] = in ? a.sc[(size_t)sc_ * Wn + (m >> 6)] : 0ull;
            hin[q] = in ? s.hmat[(size_t)svc_ * N + n] : 0u;
            if (!SCAN_CM) ein[q] = in ? s.emat[(size_t)svc_ * N + n] : LIST_EMPTY;
            lfn[q] = in ? p.leaf_of_node[(size_t)tree_ * a.n_nodes + m] : LIST_EMPTY;
        }
    };
    // SCAN_CM: a node's list entry is read by the owner of the pick only, behind the task's second barrier — it is requested at the END of
    // the turn before (it has a whole turn to arrive), so that no copy of the current task's entries has to be kept while the next
    // task's are under way: four nodes a thread leave no registers for one.
    auto ahead_entries = [&](u32 svc_) {
        WV_UNROLL
        for (int q = 0; q < SCAN_NQ; ++q) {
            const u32 n = tid + (u32)q * SCAN_THREADS;
            ein[q] = ((present >> q) & 1u) ? s.emat[(size_t)svc_ * N + n] : LIST_EMPTY;
        }
    };
    ahead(sc_n, svc_n, tree_n);
    if (SCAN_CM) ahead_entries(svc_n);
    // SCAN_CM: the base row of the NEXT task's pair is stored where that task's set is cleared, in front of this task's first barrier.
    // It is requested a task ahead of the store (bn: this thread's word of the row, i = tid — a tree of more than SCAN_THREADS branches
    // reads the words beyond from global memory in place), and the pair that says which row a task before that (pr_nn), with sc / svc / tree.
    u32 bn = 0, pr_nn = 0;
    if (SCAN_CM) {
        bn = tid < M ? p.base[(size_t)p.tpair[second] * M + tid] : 0u;   // the row of task j0 + 1, stored in task j0's turn
        pr_nn = p.tpair[s.j0 + 2u < s.j1 ? s.j0 + 2u : last];           // the pair of task j0 + 2: its row is requested in task j0's turn
    }
    wv::barrier();
    for (u32 t = s.j0; t < s.j1; ++t) {
        const RTask r = a.rt[t];   // (its cache line was touched two tasks ago, for the three words)
        const u32 set = (t - s.j0) & 1u, tree = tree_n, tbase = l_off[tree], ntn = l_off[tree + 1] - tbase;
        u32 hiq[SCAN_NQ], enq[SCAN_NQ];   // (the owner of the pick needs its key half and list entry again)
        WV_UNROLL
        for (int q = 0; q < SCAN_NQ; ++q) { hiq[q] = hin[q]; if (!SCAN_CM) enq[q] = ein[q]; }
        u64* leafmin = lmin + (size_t)set * M;
        u32* tsum = lsum + (size_t)set * M;
        u32* noroom = lnor + (size_t)set * M;
        const u32 gset = a.n_rg ? a.tg[t] : 0u;
        u32 fix_c = LIST_EMPTY, fix_e = LIST_EMPTY;   // SCAN_CM: the row this thread placed a task of the NEXT task's service on, and its list entry
        // the next task's set (last read by the walk two tasks ago, in front of that task's second barrier)
        if (!SCAN_CM)
            for (u32 i = tid; i < M; i += SCAN_THREADS) { lmin[(size_t)(set ^ 1u) * M + i] = KEY_NONE; lsum[(size_t)(set ^ 1u) * M + i] = 0; lnor[(size_t)(set ^ 1u) * M + i] = 0; }
        else {
            const u32* bx = p.base + (size_t)p.tpair[t + 1u < s.j1 ? t + 1u : last] * M;   // (read beyond SCAN_THREADS branches only)
            for (u32 i = tid; i < M; i += SCAN_THREADS) { lmin[(size_t)(set ^ 1u) * M + i] = KEY_NONE; lsum[(size_t)(set ^ 1u) * M + i] = i == tid ? bn : bx[i]; lnor[(size_t)(set ^ 1u) * M + i] = 0; }
            bn = tid < M ? p.base[(size_t)pr_nn * M + tid] : 0u;   // the row of task t + 2
            pr_nn = p.tpair[t + 3u < s.j1 ? t + 3u : last];
        }
        // ---- every thread: its nodes into their leaves
        WV_UNROLL
        for (int q = 0; q < SCAN_NQ; ++q) {
            const u32 n = tid + (u32)q * SCAN_THREADS, m = SCAN_CM ? real[q] : n;   // n: the row (SCAN_CM: the compact index), m: the node
            if (!((present >> q) & 1u)) continue;
            const u32 w = m >> 6;
            const u64 bit = 1ull << (m & 63);
            const u32 hi = hiq[q], lf = lfn[q];
            if (lf >= ntn) continue;   // (tables of another nodeSet: the launcher builds them from the one the batch was prepared for)
            if (hi & 0xFFFFFFu) wv::lds_add32(tsum + lf, hi & 0xFFFFFFu);   // tree.tasks: every node of the nodeSet, feasible or not
            if (SCAN_CM ? !((scn[q] >> (m & 31u)) & 1u) : !(scn[q] & bit)) continue;   // (the static class row holds valid & ready & constraints & platform & plugins)
            if ((r.flags & RT_RES) && !(r.cpu <= cpu[n] && r.mem <= mem[n])) continue;
            bool ok = true;
            if (gset)
                for (u32 g = a.gs_off[gset]; g < a.gs_off[gset + 1]; ++g) {
                    const u32 row = a.gs_row[g];
                    if (a.gcnt[(size_t)a.rg_kind[row] * a.gstride + m] < a.rg_val[row]) ok = false;   // HasEnough, validate.go:24-52
                }
            if (ok && (r.flags & RT_PORTS))
                for (u32 z = a.pset_off[r.pset]; z < a.pset_off[r.pset + 1]; ++z)
                    if (wv::g_fresh64(a.portmap + (size_t)a.pset_ids[z] * Wn + w) & bit) ok = false;
            if (ok && (r.flags & RT_MAXREP) && !((u64)(hi & 0xFFFFFFu) < r.maxrep)) ok = false;
            if (!ok) continue;
            const u32 tn = tot[n];
            if (tn >> 20) a.blk->error = ERR_LEVEL_RANGE;   // (beyond the 20 bits the packed key has for the count)
            wv::lds_min64(leafmin + lf, ((u64)hi << 32) | ((u64)tn << 12) | n);
        }
        // the next task's words are requested now: they have the rest of this task's turn to arrive
        sc_n = sc_nn;
        svc_n = svc_nn;
        tree_n = tree_nn;
        if (t + 1 < s.j1) ahead(sc_n, svc_n, tree_n);
        {
            const u32 t2 = t + 2 < s.j1 ? t + 2 : last;
            sc_nn = a.rt[t2].sc;
            svc_nn = a.rt[t2].svc;
            tree_nn = p.ttree[t2];
        }
        wv::barrier();
        // ---- wave 0: the sums up the tree, a level at a time from the deepest (a child's sum is complete before it is added), then the walk
        if (tid < 64) {
            for (u32 d = p.max_depth; d >= 1; --d) {
                for (u32 i = lane; i < ntn; i += 64)
                    if (l_depth[tbase + i] == d && tsum[i]) wv::lds_add32(tsum + l_parent[tbase + i], tsum[i]);
                wv::wave_sync();
                wv::lockstep();
            }
            if (lane == 0) {
                bool hang = false;
                res[set] = spread_walk(l_first + tbase, l_next + tbase, l_nchild + tbase, p.max_depth, ntn, leafmin, tsum, noroom, frames, &hang);
                if (hang) a.blk->error = ERR_SPREAD_WALK;
            }
        }
        wv::barrier();
        const u64 gk = wv::lds_read64(res + set);
        const u32 gn = gk == KEY_NONE ? R6_NONE : (u32)gk & 0xFFFu;
        // ---- the owner of the node applies the placement (NodeInfo.addTask); everybody counts
        if (gn == R6_NONE) {
            if (tid == 0) {
                a.inf_task[ni] = t;
                a.inf_pos[ni] = nc;
                a.out_node[t] = -1;
            }
            ++ni;
        } else {
            if ((gn & (SCAN_THREADS - 1u)) == tid) {
                const u32 nd = gn;
                u32 m = nd;   // the node behind the row
                if (SCAN_CM) {
                    WV_UNROLL
                    for (int q = 0; q < SCAN_NQ; ++q)
                        if (tid + (u32)q * SCAN_THREADS == nd) m = real[q];
                }
                const u32 w = m >> 6;
                const u64 bit = 1ull << (m & 63);
                if (r.cpu) cpu[nd] -= r.cpu;
                if (r.mem) mem[nd] -= r.mem;
                if (gset)
                    for (u32 g = a.gs_off[gset]; g < a.gs_off[gset + 1]; ++g) a.gcnt[(size_t)a.rg_kind[a.gs_row[g]] * a.gstride + m] -= a.rg_val[a.gs_row[g]];   // Claim
                if (r.flags & RT_PORTS)
                    for (u32 q = a.pset_off[r.pset]; q < a.pset_off[r.pset + 1]; ++q) wv::g_or64(a.portmap + (size_t)a.pset_ids[q] * Wn + w, bit);
                if (!(r.flags & RT_UNCOUNTED)) {
                    tot[nd] += 1;
                    u32 hi = 0, entry = LIST_EMPTY;
                    WV_UNROLL
                    for (int q = 0; q < SCAN_NQ; ++q)
                        if (tid + (u32)q * SCAN_THREADS == nd) { hi = hiq[q]; entry = SCAN_CM ? ein[q] : enq[q]; }
                    if (SCAN_CM) hi = (u32)(gk >> 32);   // (the pick's key carries its key half: hiq is not kept past the evaluation)
                    hi += 1u;
                    if ((hi & 0xFFFFFFu) == 0) a.blk->error = ERR_GROUP_RANGE;
                    s.hmat[(size_t)r.svc * N + nd] = hi;
                    if (entry == LIST_EMPTY) {
                        wv::g_or64(a.X + (size_t)r.svc * a.xs + w, bit);
                        a.list_node[r.slot] = m;
                        a.list_svc[r.slot] = 1;
                        a.list_fail[r.slot] = 0;
                        s.emat[(size_t)r.svc * N + nd] = r.slot;
                        entry = r.slot;
                    } else
                        a.list_svc[entry] = hi & 0xFFFFFFu;   // (the entry's count is the key half's low 24 bits)
                    if (svc_n == r.svc) {   // the next task is of the same service: what it read of this node is a placement old
                        WV_UNROLL
                        for (int q = 0; q < SCAN_NQ; ++q)
                            if (tid + (u32)q * SCAN_THREADS == nd) { hin[q] = hi; if (!SCAN_CM) ein[q] = entry; }
                        if (SCAN_CM) { fix_c = nd; fix_e = entry; }
                    }
                }
                const int32_t prev = lastc[nd];
                a.log_node[nc] = m;
                a.log_task[nc] = t;
                a.log_prev[nc] = prev;
                lastc[nd] = (int32_t)nc;
                a.out_node[t] = (int32_t)m;
            }
            ++nc;
        }
        if (SCAN_CM && t + 1 < s.j1) {   // the next task's list entries (the cell this thread has just written: from the register)
            ahead_entries(svc_n);
            WV_UNROLL
            for (int q = 0; q < SCAN_NQ; ++q)
                if (tid + (u32)q * SCAN_THREADS == fix_c) ein[q] = fix_e;
        }
        // (no third barrier: a node's row and its matrix cells are read and written by its owner only; the per-tree words alternate)
    }
    if (!SCAN_CM)
        for (u32 n = tid; n < N; n += SCAN_THREADS) { a.cpu[n] = cpu[n]; a.mem[n] = mem[n]; a.total[n] = tot[n]; a.last[n] = lastc[n]; }
    else {   // the union's nodes only: no other node was read, none is written
        WV_UNROLL
        for (int q = 0; q < SCAN_NQ; ++q) {
            const u32 n = tid + (u32)q * SCAN_THREADS, m = real[q];
            if (n < N) { a.cpu[m] = cpu[n]; a.mem[m] = mem[n]; a.total[m] = tot[n]; a.last[m] = lastc[n]; }
        }
    }
    if (tid == 0) {
        a.ctl->ncommit = nc;
        a.ctl->ninf = ni;
        a.blk->pos = s.j1;
    }
}
#endif   // SWP_SCAN_SPREAD_KERNEL

// The WIDE instance: k_scan_spread<.., false>'s semantics over ALL a.n_nodes slots of a nodeSet beyond SCAN_MAXN — the task with
// preferences and no constraint, whose own class row holds every ready node. What stops the plain instance is where it keeps its state:
// here the node rows (cpu, mem, total, last) STAY in global memory, read and written in place by their owner (thread tid owns the nodes
// tid, tid + SCAN_THREADS, ... — up to 64 of them: `present` is one bit a node), so there is no prologue copy and no epilogue copy, and
// LDS holds only the result words, the two sets of per-tree words, the frames and the trees' tables (scan_lds_spw). No per-node copies
// of the next task's words either: the class word, the hmat cell, the leaf and the row of a node are read inside the loop over the
// thread's nodes, SPW_U nodes at a time so that the loads of SPW_U iterations are in flight together; only the three words that say
// where a task's data lies (sc, svc, tree) are requested two tasks ahead. A plain thread issues up to four LDS atomics a task, a wide
// one would issue up to 64 on a handful of leaf words: the running sum and the least key are FOLDED in registers while consecutive
// nodes of the thread fall into the same leaf, and an atomic is issued only when the leaf changes and at the loop's end (exact: min and
// add are associative and the key carries the node). The key is hi << 32 | total << 16 | node: SPREAD_WIDE_MAXN = 65 536 slots, and a
// feasible node that holds 65 536 tasks or more raises ERR_LEVEL_RANGE and STOPS the segment in front of the task (a word in LDS, read
// by everybody behind the task's first barrier: the trip count stays uniform) — never a wrong pick. No base sums: nothing lies outside
// the node range (tpair / base stay null).
#define SPREAD_WIDE_MAXN 65536u
#define SPW_U 4
// two result words, the stop word + two sets of (leafmin, tsum, noroom) per tree node of the largest tree + a frame per level + the tables
inline __host__ __device__ size_t scan_lds_spw(u32 max_ntn, u32 max_depth, u32 n_trees, u32 tot_ntn) {
    return 32 + (size_t)2 * max_ntn * 16 + (size_t)(max_depth + 1) * sizeof(SpFrame) + ((size_t)n_trees + 1 + (size_t)5 * tot_ntn) * 4;
}

#ifdef SWP_SCAN_SPREAD_KERNEL
WV_KERNEL(SCAN_THREADS) void k_scan_spread_wide(SpreadArgs p) {
    const ScanArgs& s = p.s;
    const R6Args& a = s.a;
    const u32 tid = wv::tid(), lane = wv::lane(), N = a.n_nodes, Wn = a.n_words, M = p.max_ntn;
    u64* res = wv::lds();                                  // [2] the walk's answer, alternating; [2]: != 0 stops the segment
    u64* lmin = res + 4;                                   // [2][M] a leaf's least key
    u32* lsum = reinterpret_cast<u32*>(lmin + 2 * (size_t)M);   // [2][M] tree.tasks
    u32* lnor = lsum + 2 * (size_t)M;                      // [2][M] noRoom
    SpFrame* frames = reinterpret_cast<SpFrame*>(lnor + 2 * (size_t)M);   // [max_depth + 1]
    u32* l_off = reinterpret_cast<u32*>(frames + p.max_depth + 1);       // [n_trees + 1] tree_off
    u32* l_parent = l_off + p.n_trees + 1;                                // [tot_ntn] each: the trees' tables
    u32* l_first = l_parent + p.tot_ntn;
    u32* l_next = l_first + p.tot_ntn;
    u32* l_nchild = l_next + p.tot_ntn;
    u32* l_depth = l_nchild + p.tot_ntn;
    if (a.blk->error != ERR_NONE) return;
    const u32 last = s.j0 < s.j1 ? s.j1 - 1u : 0u, first = s.j0 < s.j1 ? s.j0 : 0u;   // (reads beyond the stretch are clamped to its last task and never used)
    const u32 second = s.j0 + 1u < s.j1 ? s.j0 + 1u : last;
    for (u32 i = tid; i < 2 * M; i += SCAN_THREADS) { lmin[i] = KEY_NONE; lsum[i] = 0; lnor[i] = 0; }
    if (tid == 0) res[2] = 0;
    for (u32 i = tid; i <= p.n_trees; i += SCAN_THREADS) l_off[i] = p.tree_off[i];
    for (u32 i = tid; i < p.tot_ntn; i += SCAN_THREADS) {
        l_parent[i] = p.tn_parent[i]; l_first[i] = p.tn_first[i]; l_next[i] = p.tn_next[i]; l_nchild[i] = p.tn_nchild[i]; l_depth[i] = p.tn_depth[i];
    }
    const u32 nq = (N + SCAN_THREADS - 1u) / SCAN_THREADS;   // nodes of the thread with the most (<= 64: the launcher refuses more slots)
    u64 present = 0;   // bit q: this thread's q-th node exists and is in the nodeSet
    for (u32 q = 0; q < nq; ++q) {
        const u32 n = tid + q * SCAN_THREADS;
        if (n < N && ((a.valid[n >> 6] >> (n & 63)) & 1ull)) present |= 1ull << q;
    }
    u32 nc = a.ctl->ncommit, ni = a.ctl->ninf;
    u32 sc_n = a.rt[first].sc, svc_n = a.rt[first].svc, tree_n = p.ttree[first];
    u32 sc_nn = a.rt[second].sc, svc_nn = a.rt[second].svc, tree_nn = p.ttree[second];
    const u32* sc32 = reinterpret_cast<const u32*>(a.sc);   // (the class word as the 32-bit half that holds the node's bit)
    wv::barrier();
    u32 t = s.j0;
    for (; t < s.j1; ++t) {
        const RTask r = a.rt[t];
        const u32 set = (t - s.j0) & 1u, tree = tree_n, tbase = l_off[tree], ntn = l_off[tree + 1] - tbase;
        const u32 sc_t = sc_n, svc_t = svc_n;
        u64* leafmin = lmin + (size_t)set * M;
        u32* tsum = lsum + (size_t)set * M;
        u32* noroom = lnor + (size_t)set * M;
        const u32 gset = a.n_rg ? a.tg[t] : 0u;
        const bool with_res = (r.flags & RT_RES) != 0;
        // the next task's set (last read by the walk two tasks ago, in front of that task's second barrier)
        for (u32 i = tid; i < M; i += SCAN_THREADS) { lmin[(size_t)(set ^ 1u) * M + i] = KEY_NONE; lsum[(size_t)(set ^ 1u) * M + i] = 0; lnor[(size_t)(set ^ 1u) * M + i] = 0; }
        // the words that say where the tasks behind this one lie: they have this task's whole turn to arrive
        sc_n = sc_nn;
        svc_n = svc_nn;
        tree_n = tree_nn;
        {
            const u32 t2 = t + 2 < s.j1 ? t + 2 : last;
            sc_nn = a.rt[t2].sc;
            svc_nn = a.rt[t2].svc;
            tree_nn = p.ttree[t2];
        }
        // ---- every thread: its nodes into their leaves, SPW_U at a time; the fold runs across the groups
        const u32* scrow = sc32 + (size_t)sc_t * Wn * 2u;
        const u32* hrow = s.hmat + (size_t)svc_t * N;
        const u32* lrow = p.leaf_of_node + (size_t)tree * N;
        u32 cur = 0, acc = 0;   // the leaf of the fold, its sum so far ...
        u64 best = KEY_NONE;    // ... and its least key so far
        for (u32 q0 = 0; q0 < nq; q0 += SPW_U) {
            const u32 pm = (u32)(present >> q0) & ((1u << SPW_U) - 1u);
            if (!pm) continue;
            u32 scw[SPW_U], hiv[SPW_U], lfv[SPW_U], ttv[SPW_U];
            i64 cpv[SPW_U], mmv[SPW_U];
            WV_UNROLL
            for (int i = 0; i < SPW_U; ++i) {
                const u32 n = tid + (q0 + (u32)i) * SCAN_THREADS;
                const bool in = (pm >> i) & 1u;
                scw[i] = in ? scrow[n >> 5] : 0u;
                hiv[i] = in ? hrow[n] : 0u;
                lfv[i] = in ? lrow[n] : LIST_EMPTY;
                ttv[i] = in ? a.total[n] : 0u;
                cpv[i] = in && with_res ? a.cpu[n] : 0;
                mmv[i] = in && with_res ? a.mem[n] : 0;
            }
            WV_UNROLL
            for (int i = 0; i < SPW_U; ++i) {
                if (!((pm >> i) & 1u)) continue;
                const u32 n = tid + (q0 + (u32)i) * SCAN_THREADS, w = n >> 6;
                const u64 bit = 1ull << (n & 63);
                const u32 hi = hiv[i], lf = lfv[i];
                if (lf >= ntn) continue;   // (tables of another nodeSet: the launcher builds them from the one the batch was prepared for)
                if (lf != cur) {           // the leaf changes: what the fold holds goes to LDS
                    if (acc) wv::lds_add32(tsum + cur, acc);
                    if (best != KEY_NONE) wv::lds_min64(leafmin + cur, best);
                    cur = lf;
                    acc = 0;
                    best = KEY_NONE;
                }
                acc += hi & 0xFFFFFFu;     // tree.tasks: every node of the nodeSet, feasible or not
                if (!((scw[i] >> (n & 31u)) & 1u)) continue;   // (the static class row holds valid & ready & constraints & platform & plugins)
                if (with_res && !(r.cpu <= cpv[i] && r.mem <= mmv[i])) continue;
                bool ok = true;
                if (gset)
                    for (u32 g = a.gs_off[gset]; g < a.gs_off[gset + 1]; ++g) {
                        const u32 row = a.gs_row[g];
                        if (a.gcnt[(size_t)a.rg_kind[row] * a.gstride + n] < a.rg_val[row]) ok = false;   // HasEnough, validate.go:24-52
                    }
                if (ok && (r.flags & RT_PORTS))
                    for (u32 z = a.pset_off[r.pset]; z < a.pset_off[r.pset + 1]; ++z)
                        if (wv::g_fresh64(a.portmap + (size_t)a.pset_ids[z] * Wn + w) & bit) ok = false;
                if (ok && (r.flags & RT_MAXREP) && !((u64)(hi & 0xFFFFFFu) < r.maxrep)) ok = false;
                if (!ok) continue;
                const u32 tn = ttv[i];
                if (tn >> 16) {   // beyond the 16 bits the key has for the count: the segment stops in front of this task
                    a.blk->error = ERR_LEVEL_RANGE;
                    res[2] = 1;
                    continue;
                }
                const u64 key = ((u64)hi << 32) | ((u64)tn << 16) | n;
                if (key < best) best = key;
            }
        }
        if (acc) wv::lds_add32(tsum + cur, acc);
        if (best != KEY_NONE) wv::lds_min64(leafmin + cur, best);
        wv::barrier();
        if (wv::lds_read64(res + 2)) break;   // (written in front of the barrier only, never cleared: uniform)
        // ---- wave 0: the sums up the tree, a level at a time from the deepest (a child's sum is complete before it is added), then the walk
        if (tid < 64) {
            for (u32 d = p.max_depth; d >= 1; --d) {
                for (u32 i = lane; i < ntn; i += 64)
                    if (l_depth[tbase + i] == d && tsum[i]) wv::lds_add32(tsum + l_parent[tbase + i], tsum[i]);
                wv::wave_sync();
                wv::lockstep();
            }
            if (lane == 0) {
                bool hang = false;
                res[set] = spread_walk(l_first + tbase, l_next + tbase, l_nchild + tbase, p.max_depth, ntn, leafmin, tsum, noroom, frames, &hang);
                if (hang) a.blk->error = ERR_SPREAD_WALK;
            }
        }
        wv::barrier();
        const u64 gk = wv::lds_read64(res + set);
        const u32 gn = gk == KEY_NONE ? R6_NONE : (u32)gk & (SPREAD_WIDE_MAXN - 1u);
        // ---- the owner of the node applies the placement (NodeInfo.addTask), on the node's row in global memory; everybody counts
        if (gn == R6_NONE) {
            if (tid == 0) {
                a.inf_task[ni] = t;
                a.inf_pos[ni] = nc;
                a.out_node[t] = -1;
            }
            ++ni;
        } else {
            if ((gn & (SCAN_THREADS - 1u)) == tid) {
                const u32 nd = gn, w = nd >> 6;
                const u64 bit = 1ull << (nd & 63);
                if (r.cpu) a.cpu[nd] -= r.cpu;
                if (r.mem) a.mem[nd] -= r.mem;
                if (gset)
                    for (u32 g = a.gs_off[gset]; g < a.gs_off[gset + 1]; ++g) a.gcnt[(size_t)a.rg_kind[a.gs_row[g]] * a.gstride + nd] -= a.rg_val[a.gs_row[g]];   // Claim
                if (r.flags & RT_PORTS)
                    for (u32 q = a.pset_off[r.pset]; q < a.pset_off[r.pset + 1]; ++q) wv::g_or64(a.portmap + (size_t)a.pset_ids[q] * Wn + w, bit);
                if (!(r.flags & RT_UNCOUNTED)) {
                    a.total[nd] += 1;
                    const u32 hi = (u32)(gk >> 32) + 1u;   // (the pick's key carries its key half)
                    u32 entry = s.emat[(size_t)r.svc * N + nd];
                    if ((hi & 0xFFFFFFu) == 0) a.blk->error = ERR_GROUP_RANGE;
                    s.hmat[(size_t)r.svc * N + nd] = hi;
                    if (entry == LIST_EMPTY) {
                        wv::g_or64(a.X + (size_t)r.svc * a.xs + w, bit);
                        a.list_node[r.slot] = nd;
                        a.list_svc[r.slot] = 1;
                        a.list_fail[r.slot] = 0;
                        s.emat[(size_t)r.svc * N + nd] = r.slot;
                    } else
                        a.list_svc[entry] = hi & 0xFFFFFFu;   // (the entry's count is the key half's low 24 bits)
                    // (the plain instance corrects the next task's copy of this cell here. There is no copy: this thread stores the
                    // cell and loads it again, in the next task's loop over its nodes, in program order.)
                }
                const int32_t prev = a.last[nd];
                a.log_node[nc] = nd;
                a.log_task[nc] = t;
                a.log_prev[nc] = prev;
                a.last[nd] = (int32_t)nc;
                a.out_node[t] = (int32_t)nd;
            }
            ++nc;
        }
        // (no third barrier: a node's row and its matrix cells are read and written by its owner only; the per-tree words alternate)
    }
    if (tid == 0) {
        a.ctl->ncommit = nc;
        a.ctl->ninf = ni;
        a.blk->pos = t;   // (s.j1, or the task the segment stopped in front of)
    }
}
#endif   // SWP_SCAN_SPREAD_KERNEL

}  // namespace swpdev
