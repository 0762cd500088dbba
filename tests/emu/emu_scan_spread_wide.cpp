// emu_scan_spread_wide.cpp — runs the WIDE spread instance of the scan resolver (swarmkit_amd/csrc/swp_scan_spread.hpp:
// k_scan_spread_wide behind k_scan_fill / k_scan_lists over all nodes: the node rows in global memory, up to 64 nodes a thread, the
// register fold in front of the LDS atomics, the key hi << 32 | total << 16 | node) on CPU fibers against the sequential model of
// emu_scan_spread.cpp, copied here (written from the reference's text: nodeSet.tree with a heap of one, scheduleNTasksOnSubtree as the
// recursion it is, NodeInfo.addTask) — every output, every mutated array, and a guard zone behind every array the kernel writes.
// TEST INFRASTRUCTURE (tests/test_emu_scan_spread_wide.py); not product.
//
//   emu_scan_spread_wide <seed> <N> <T> <S> <block> <order: 0 rr | 1 major | 2 random> <features 0..3> <levels 0..3> <values per key 1..> [flags]
//   flags: v verbose | m block / spread / block in thirds (the outer thirds' tasks carry no preferences) | l a fifth of the nodes lack
//   each label (the "" branch) | d the nodes of one first-level branch fail every class (a branch without room whose nodes still carry
//   tasks; asserted) | a every label is a function of n mod 1 024: ALL nodes of a thread fall into one leaf (one fold a task) | z every
//   label is a function of n / 1 024: a thread's consecutive nodes ALTERNATE between leaves (an atomic a node) | e / E two nodes only pass
//   the class rows, 1 024 apart (5 and 1 029: one thread, the fold in registers) / 65 535 apart (0 and 65 535: two threads, the LDS
//   minimum), equal in everything: asserted that the first task takes the lower and the second the higher | h only nodes from 32 768 on
//   pass the class rows: every pick has the key's top node bit set (asserted) | t a third of the nodes hold 65 535 tasks (legal) |
//   T one node that passes everything holds 65 536 tasks: ERR_LEVEL_RANGE, the segment stops in front of the first task that could
//   take it, and everything up to there equals the model
#include "wv_emu.hpp"

#define SWP_R6_KERNELS
#include "../../swarmkit_amd/csrc/swp_resolve6.hpp"
#define SWP_SCAN_KERNELS          // (k_scan_fill, k_scan_lists: the matrices)
#define SWP_SCAN_SPREAD_KERNEL
#include "../../swarmkit_amd/csrc/swp_scan_spread.hpp"

#include "emu_model.hpp"

#include <functional>

template <class F>
static void grid(u32 blocks, u32 threads, size_t lds, F body) {
    for (u32 b = 0; b < blocks; ++b) {
        emu::blockidx() = b;
        emu::launch(threads, lds, body);
    }
    emu::blockidx() = 0;
}

// ---- the model (emu_scan_spread.cpp's) ------------------------------------------------------------------------------------------
struct MTree {   // decisionTree (decision_tree.go:8-22) with a heap of one
    i64 tasks = 0;
    std::vector<std::pair<u32, MTree*>> next;   // creation order = first seen in node order (the canonical order of the map's range)
    bool has = false;                           // nodeHeap holds a node ...
    u32 node = 0;                               // ... this one
    ~MTree() { for (auto& c : next) delete c.second; }
    MTree* child(u32 value) {
        for (auto& c : next)
            if (c.first == value) return c.second;
        next.push_back({value, new MTree()});
        return next.back().second;
    }
};
struct Model {
    const Problem& p;
    State& s;
    const std::vector<std::vector<u32>>& label;       // [key][node] value id, 0 = ""
    const std::vector<std::vector<u32>>& tree_keys;   // [tree] the spread levels' keys
    std::vector<std::map<u32, u32>> entry;            // [service] node -> list entry
    u64 noroom_events = 0, spread_placed = 0, spread_unplaced = 0, handed_more = 0;
    bool group_left = true;                           // the group map still holds the task
    int32_t picked = -1;
    Model(const Problem& p_, State& s_, const std::vector<std::vector<u32>>& l, const std::vector<std::vector<u32>>& tk) : p(p_), s(s_), label(l), tree_keys(tk), entry(p_.S) {
        for (u32 sv = 0; sv < p.S; ++sv)
            for (u32 e = p.list_off[sv]; e < p.list_off[sv + 1]; ++e)
                if (s.list_node[e] != LIST_EMPTY) entry[sv][s.list_node[e]] = e;
    }
    u32 count(u32 sv, u32 n) const { auto it = entry[sv].find(n); return it == entry[sv].end() ? 0u : s.list_svc[it->second]; }
    u32 fails(u32 sv, u32 n) const { auto it = entry[sv].find(n); return it == entry[sv].end() ? 0u : s.list_fail[it->second]; }
    bool process(u32 j, u32 n) const {   // the pipeline against the state NOW
        const RTask& r = p.rt[j];
        if (!((p.sc[(size_t)r.sc * p.Wn + (n >> 6)] >> (n & 63)) & 1)) return false;
        if ((r.flags & RT_RES) && !(r.cpu <= s.cpu[n] && r.mem <= s.mem[n])) return false;
        if ((r.flags & RT_RES) && p.lacks(s.gcnt, j, n)) return false;
        if (r.flags & RT_PORTS)
            for (u32 q = p.pset_off[r.pset]; q < p.pset_off[r.pset + 1]; ++q)
                if ((s.portmap[(size_t)p.pset_ids[q] * p.Wn + (n >> 6)] >> (n & 63)) & 1) return false;
        if ((r.flags & RT_MAXREP) && !((u64)count(r.svc, n) < r.maxrep)) return false;
        return true;
    }
    bool node_less(u32 sv, u32 a, u32 b) const {   // scheduler.go:708-735
        const u32 fa = fails(sv, a), fb = fails(sv, b);
        if (fa >= MAX_FAILURES || fb >= MAX_FAILURES) {
            if (fa > fb) return false;
            if (fb > fa) return true;
        }
        const u32 ca = count(sv, a), cb = count(sv, b);
        if (ca < cb) return true;
        if (ca > cb) return false;
        return s.total[a] < s.total[b];
    }
    void add_task(u32 j, u32 n) {
        const RTask& r = p.rt[j];
        s.cpu[n] -= r.cpu;
        s.mem[n] -= r.mem;
        if (!p.tg.empty())
            for (u32 g = p.gs_off[p.tg[j]]; g < p.gs_off[p.tg[j] + 1]; ++g) s.gcnt[(size_t)p.rg_kind[p.gs_row[g]] * p.N + n] -= p.rg_val[p.gs_row[g]];
        if (r.flags & RT_PORTS)
            for (u32 q = p.pset_off[r.pset]; q < p.pset_off[r.pset + 1]; ++q) s.portmap[(size_t)p.pset_ids[q] * p.Wn + (n >> 6)] |= 1ull << (n & 63);
        if (!(r.flags & RT_UNCOUNTED)) {
            s.total[n] += 1;
            auto it = entry[r.svc].find(n);
            if (it == entry[r.svc].end()) {
                s.X[(size_t)r.svc * p.Wn + (n >> 6)] |= 1ull << (n & 63);
                s.list_node[r.slot] = n;
                s.list_svc[r.slot] = 1;
                s.list_fail[r.slot] = 0;
                entry[r.svc][n] = r.slot;
            } else
                s.list_svc[it->second] += 1;
        }
        const u32 ci = s.ctl.ncommit++;
        s.log_node[ci] = n;
        s.log_task[ci] = j;
        s.log_prev[ci] = s.last[n];
        s.last[n] = (int32_t)ci;
        s.out[j] = (int32_t)n;
    }
    // scheduleNTasksOnSubtree; the leaf case is scheduleNTasksOnNodes over a group map of one task (an empty map: its loop does not run)
    i64 on_subtree(u32 j, i64 n, MTree* tree) {
        if (tree->next.empty()) {
            if (!tree->has) return 0;
            if (!group_left) return 0;
            picked = (int32_t)tree->node;
            add_task(j, tree->node);
            group_left = false;
            return 1;
        }
        i64 scheduled = 0, usable = tree->tasks;
        std::set<MTree*> no_room;
        bool converging = true;
        u64 guard = 0;
        while (scheduled != n && no_room.size() != tree->next.size() && converging) {
            if (++guard > 1000000) { fprintf(stderr, "the model's walk does not end\n"); exit(4); }
            const i64 room = (i64)tree->next.size() - (i64)no_room.size();
            const i64 desired = (usable + n - scheduled) / room;
            i64 rem = (usable + n - scheduled) % room;
            converging = false;
            for (auto& c : tree->next) {
                MTree* sub = c.second;
                if (no_room.count(sub)) continue;
                if (sub->tasks < desired || (sub->tasks == desired && rem > 0)) {
                    converging = true;
                    i64 assign = desired - sub->tasks;
                    if (rem > 0) assign++;
                    if (assign > 1 && group_left) handed_more++;
                    const i64 res = on_subtree(j, assign, sub);
                    if (res < assign) {
                        if (group_left) noroom_events++;   // (behind the placement every call returns 0: those are not branches without room)
                        no_room.insert(sub);
                        usable -= sub->tasks;
                    } else if (rem > 0)
                        rem--;
                    scheduled += res;
                }
            }
        }
        return scheduled;
    }
    void task(u32 j, u32 tree_id) {
        const RTask& r = p.rt[j];
        MTree root;
        for (u32 n = 0; n < p.N; ++n) {   // nodeSet.tree, maxAssignments = 1
            if (!((p.valid[n >> 6] >> (n & 63)) & 1)) continue;
            MTree* t = &root;
            for (u32 key : tree_keys[tree_id]) {
                t->tasks += count(r.svc, n);
                t = t->child(label[key][n]);
            }
            t->tasks += count(r.svc, n);
            if (!t->has) {
                if (process(j, n)) { t->has = true; t->node = n; }
            } else if (node_less(r.svc, n, t->node)) {
                if (process(j, n)) t->node = n;
            }
        }
        group_left = true;
        picked = -1;
        on_subtree(j, 1, &root);
        if (group_left) {   // noSuitableNode
            s.inf_task[s.ctl.ninf] = j;
            s.inf_pos[s.ctl.ninf] = s.ctl.ncommit;
            s.ctl.ninf++;
            if (!tree_keys[tree_id].empty()) spread_unplaced++;
        } else if (!tree_keys[tree_id].empty())
            spread_placed++;
    }
};

// a guard zone behind an array: GUARD elements of a pattern, appended to the kernel's copy and to the model's alike
constexpr size_t GUARD = 64;
static std::vector<std::function<bool()>> g_guards;
template <class T>
static void guard(const char* what, std::vector<T>& v) {
    const size_t n0 = v.size();
    T pat;
    memset(&pat, 0x5A, sizeof pat);
    v.insert(v.end(), GUARD, pat);
    std::vector<T>* pv = &v;
    g_guards.push_back([what, pv, n0, pat]() {
        for (size_t i = n0; i < n0 + GUARD; ++i)
            if (memcmp(&(*pv)[i], &pat, sizeof pat) != 0) { fprintf(stderr, "GUARD: %s[%zu + %zu] was written\n", what, n0, i - n0); return false; }
        return pv->size() == n0 + GUARD;
    });
}
static void guard_state(State& s) {
    guard("cpu", s.cpu); guard("mem", s.mem); guard("total", s.total); guard("X", s.X); guard("portmap", s.portmap);
    guard("list_node", s.list_node); guard("list_svc", s.list_svc); guard("list_fail", s.list_fail);
    guard("out", s.out); guard("log_prev", s.log_prev); guard("last", s.last); guard("log_node", s.log_node); guard("log_task", s.log_task);
    guard("inf_task", s.inf_task); guard("inf_pos", s.inf_pos); guard("gcnt", s.gcnt);
}

int main(int argc, char** argv) {
    if (argc < 10) { fprintf(stderr, "usage: %s seed N T S block order features(0..3) levels(0..3) values [v] [m] [d] [l] [a] [z] [e] [E] [h] [t] [T]\n", argv[0]); return 2; }
    const u32 seed = atoi(argv[1]);
    u32 N = atoi(argv[2]), T = atoi(argv[3]), S = atoi(argv[4]);
    const u32 B = atoi(argv[5]);
    const int order = atoi(argv[6]), feat = atoi(argv[7]);
    const u32 levels = std::min(3, atoi(argv[8])), vals = std::max(1, atoi(argv[9]));
    bool verbose = false, mixed = false, dead = false, lack = false, one_leaf = false, alternate = false, tie_near = false, tie_far = false, high = false, tot_ok = false, tot_bad = false;
    for (int i = 10; i < argc; ++i) {
        if (argv[i][0] == 'v') verbose = true;
        if (argv[i][0] == 'm') mixed = true;
        if (argv[i][0] == 'd') dead = true;
        if (argv[i][0] == 'l') lack = true;
        if (argv[i][0] == 'a') one_leaf = true;
        if (argv[i][0] == 'z') alternate = true;
        if (argv[i][0] == 'e') tie_near = true;
        if (argv[i][0] == 'E') tie_far = true;
        if (argv[i][0] == 'h') high = true;
        if (argv[i][0] == 't') tot_ok = true;
        if (argv[i][0] == 'T') tot_bad = true;
    }
    if (N == 0 || N > SPREAD_WIDE_MAXN) { fprintf(stderr, "the wide instance takes %u nodes\n", SPREAD_WIDE_MAXN); return 2; }
    const bool tie = tie_near || tie_far;
    const u32 tie_lo = tie_far ? 0u : 5u, tie_hi = tie_far ? 65535u : 1029u;
    if (tie && (N <= tie_hi || T < 2 || feat != 0)) { fprintf(stderr, "flags e / E need the two nodes, two tasks and feature level 0\n"); return 2; }
    if (high && N <= 32768) { fprintf(stderr, "flag h needs more than 32 768 nodes\n"); return 2; }
    if (tot_bad && feat != 0) { fprintf(stderr, "flag T needs feature level 0\n"); return 2; }
    Problem p = make_problem(seed, N, T, S, order, feat);
    // labels and trees: a generator of their own (make_problem's stream is not touched)
    std::mt19937_64 g(0xA0761D6478BD642Full * (seed + 1) + 0x5B);
    auto rnd = [&](u32 k) { return (u32)(g() % k); };
    std::vector<std::vector<u32>> label(3, std::vector<u32>(N, 0));
    for (u32 k = 0; k < 3; ++k)
        for (u32 n = 0; n < N; ++n) {
            label[k][n] = (lack && rnd(5) == 0) ? 0u : 1 + rnd(vals);
            if (one_leaf) label[k][n] = 1 + ((n % SCAN_THREADS) * (k + 1)) % vals;      // the thread decides the leaf
            if (alternate) label[k][n] = 1 + ((n / SCAN_THREADS) + k) % vals;           // the thread's q-th node decides it
        }
    std::vector<std::vector<u32>> tree_keys(1);   // tree 0: no preferences
    for (u32 t = 1; t <= levels; ++t) {
        std::vector<u32> keys;
        for (u32 q = 0; q < t; ++q) keys.push_back((t - 1 + q) % 3);
        tree_keys.push_back(keys);
    }
    std::vector<u32> svc_tree(S), ttree(T);
    for (u32 s = 0; s < S; ++s) svc_tree[s] = levels ? 1 + rnd(levels) : 0u;
    for (u32 j = 0; j < T; ++j) {
        ttree[j] = rnd(5) == 0 ? 0u : svc_tree[p.rt[j].svc];   // (one service with and without preferences)
        if (mixed && (j < T / 3 || j >= 2 * T / 3)) ttree[j] = 0;
    }
    auto set_bit = [&](std::vector<u64>& v, size_t row, u32 n, bool on) {
        if (on) v[row * p.Wn + (n >> 6)] |= 1ull << (n & 63);
        else v[row * p.Wn + (n >> 6)] &= ~(1ull << (n & 63));
    };
    if (dead)   // the nodes of the first key's value 1 fail every class; they stay in the nodeSet and keep their tasks
        for (u32 c = 0; c < p.n_sc; ++c)
            for (u32 n = 0; n < N; ++n)
                if (label[0][n] == 1) set_bit(p.sc, c, n, false);
    if (high)
        for (u32 c = 0; c < p.n_sc; ++c)
            for (u32 n = 0; n < 32768; ++n) set_bit(p.sc, c, n, false);
    if (tie) {   // two nodes pass, equal in everything and in one leaf; the tasks ask for nothing they lack
        for (u32 c = 0; c < p.n_sc; ++c)
            for (u32 w = 0; w < p.Wn; ++w) p.sc[(size_t)c * p.Wn + w] = 0;
        for (u32 n : {tie_lo, tie_hi}) {
            set_bit(p.valid, 0, n, true);
            for (u32 c = 0; c < p.n_sc; ++c) set_bit(p.sc, c, n, true);
            p.cpu[n] = (i64)1 << 50;
            p.mem[n] = (i64)1 << 50;
            p.total[n] = 7;
            for (u32 k = 0; k < 3; ++k) label[k][n] = 1;
        }
        for (u32 j = 0; j < T; ++j) { p.rt[j].svc = 0; p.rt[j].sc = 0; p.rt[j].flags &= RT_RES; }
        // (feature level 0: no list entry exists, the two nodes' counts of the service are 0; every task is of service 0 — the slots
        // make_problem reserved per service do not suffice: laid out again)
        std::fill(p.X.begin(), p.X.end(), 0ull);
        p.list_off.assign(S + 1, T);
        p.list_off[0] = 0;
        p.list_node.assign(T, LIST_EMPTY);
        p.list_svc.assign(T, 0);
        p.list_fail.assign(T, 0);
        for (u32 j = 0; j < T; ++j) p.rt[j].slot = j;
        for (u32 j = 0; j < T; ++j) ttree[j] = levels ? 1u : 0u;
    }
    if (tot_ok)
        for (u32 n = 0; n < N; n += 3) p.total[n] = 65535;
    u32 bad_node = LIST_EMPTY;
    if (tot_bad) {   // a valid node of the upper half that passes every class and has room for everything
        for (u32 n = N - 1; n > 0 && bad_node == LIST_EMPTY; --n)
            if ((p.valid[n >> 6] >> (n & 63)) & 1) bad_node = n;
        if (bad_node == LIST_EMPTY) { fprintf(stderr, "flag T: no valid node\n"); return 2; }
        // (service 0's tasks only can take it: the segment stops at the first of them, not at task 0)
        const u32 row = p.n_sc;
        p.sc.resize((size_t)(p.n_sc + 1) * p.Wn);
        for (u32 w = 0; w < p.Wn; ++w) p.sc[(size_t)row * p.Wn + w] = p.sc[w];
        for (u32 c = 0; c < p.n_sc; ++c) set_bit(p.sc, c, bad_node, false);
        set_bit(p.sc, row, bad_node, true);
        p.n_sc += 1;
        for (u32 j = 0; j < T; ++j)
            if (p.rt[j].svc == S - 1) p.rt[j].sc = row;
        p.cpu[bad_node] = (i64)1 << 50;
        p.mem[bad_node] = (i64)1 << 50;
        p.total[bad_node] = 65536;
    }
    // demand classes over the raw reservations (what the engine's batch preparation does; the block resolver's stretches need them)
    std::set<i64> sc, sm;
    for (const RTask& r : p.rt)
        if (r.flags & RT_RES) { sc.insert(r.cpu); sm.insert(r.mem); }
    if (sc.size() > 255 || sm.size() > 255) { fprintf(stderr, "too many demand classes for this harness\n"); return 2; }
    std::vector<i64> thr;
    std::map<i64, u32> ic, im;
    for (i64 v : sc) { ic[v] = (u32)thr.size(); thr.push_back(v); }
    const u32 n_dc = (u32)sc.size();
    for (i64 v : sm) { im[v] = (u32)thr.size() - n_dc; thr.push_back(v); }
    const u32 n_dm = (u32)sm.size();
    for (RTask& r : p.rt)
        if (r.flags & RT_RES) r.flags |= (ic[r.cpu] << RT_DC_SHIFT) | (im[r.mem] << RT_DM_SHIFT);

    State ref = initial_state(p), em = initial_state(p);
    guard_state(em);
    {
        const size_t keep = g_guards.size();
        guard_state(ref);          // (the same lengths on both sides; only the kernel's guards are checked)
        g_guards.resize(keep);
    }
    Model model(p, ref, label, tree_keys);
    u32 stop_at = T;   // flag T: the first task that the node with 65 536 tasks passes, by the model's pipeline at that moment
    for (u32 j = 0; j < T; ++j) {
        if (tot_bad && model.process(j, bad_node)) { stop_at = j; break; }
        model.task(j, ttree[j]);
    }
    if (tot_bad && stop_at == T) { fprintf(stderr, "flag T: no task can take node %u\n", bad_node); return 2; }

    // ---- the kernel's tree tables, as the engine builds them: branches in the order their first node appears
    std::vector<u32> tree_off{0}, tn_parent, tn_first, tn_next, tn_nchild, tn_depth, leaf_of(tree_keys.size() * (size_t)N, 0xFFFFFFFFu);
    u32 max_ntn = 1, max_depth = 0;
    for (size_t t = 0; t < tree_keys.size(); ++t) {
        const u32 base = (u32)tn_parent.size();
        std::vector<u32> last_child;
        auto new_node = [&](u32 parent, u32 depth) {
            const u32 id = (u32)tn_parent.size() - base;
            tn_parent.push_back(parent); tn_first.push_back(0xFFFFFFFFu); tn_next.push_back(0xFFFFFFFFu); tn_nchild.push_back(0); tn_depth.push_back(depth);
            last_child.push_back(0xFFFFFFFFu);
            return id;
        };
        new_node(0xFFFFFFFFu, 0);
        std::map<std::pair<u32, u32>, u32> child_of;
        for (u32 n = 0; n < N; ++n) {
            if (!((p.valid[n >> 6] >> (n & 63)) & 1)) continue;
            u32 tn = 0, depth = 0;
            for (u32 key : tree_keys[t]) {
                ++depth;
                auto it = child_of.find({tn, label[key][n]});
                if (it == child_of.end()) {
                    const u32 c = new_node(tn, depth);
                    if (last_child[tn] == 0xFFFFFFFFu) tn_first[base + tn] = c;
                    else tn_next[base + last_child[tn]] = c;
                    last_child[tn] = c;
                    tn_nchild[base + tn]++;
                    it = child_of.emplace(std::make_pair(tn, label[key][n]), c).first;
                }
                tn = it->second;
            }
            leaf_of[t * N + n] = tn;
        }
        tree_off.push_back((u32)tn_parent.size());
        max_ntn = std::max(max_ntn, (u32)tn_parent.size() - base);
        max_depth = std::max(max_depth, (u32)tree_keys[t].size());
    }
    if (scan_lds_spw(max_ntn, max_depth, (u32)tree_keys.size(), tree_off.back()) > (size_t)160 * 1024 - 512) { fprintf(stderr, "the trees do not fit the LDS budget\n"); return 2; }

    std::vector<u64> planes((size_t)R6_NP * p.Wn, 0xAAAAAAAAAAAAAAAAull), rr((size_t)std::max<u32>(n_dc + n_dm, 1) * p.Wn, 0x5555555555555555ull);
    std::vector<R6Prop> prop(B);
    Blk6 blk{};
    R6Args a{};
    a.n_nodes = N;
    a.n_words = p.Wn;
    a.xs = p.Wn;
    a.block = B;
    a.n_dc = n_dc;
    a.n_dm = n_dm;
    a.valid = p.valid.data();
    a.sc = p.sc.data();
    a.X = em.X.data();
    a.rt = p.rt.data();
    a.cpu = em.cpu.data();
    a.mem = em.mem.data();
    a.total = em.total.data();
    a.list_node = em.list_node.data();
    a.list_svc = em.list_svc.data();
    a.list_fail = em.list_fail.data();
    a.list_off = p.list_off.data();
    a.portmap = em.portmap.data();
    a.pset_off = p.pset_off.data();
    a.pset_ids = p.pset_ids.data();
    a.out_node = em.out.data();
    a.log_node = em.log_node.data();
    a.log_task = em.log_task.data();
    a.log_prev = em.log_prev.data();
    a.last = em.last.data();
    a.inf_task = em.inf_task.data();
    a.inf_pos = em.inf_pos.data();
    a.ctl = &em.ctl;
    a.planes = planes.data();
    a.rr = rr.data();
    a.thr = thr.data();
    a.blk = &blk;
    a.prop = prop.data();
    std::vector<u64> trows((size_t)B * p.Wn, 0x7777777777777777ull);
    a.trows = trows.data();
    std::vector<u64> rg((size_t)std::max<size_t>(p.rg_kind.size(), 1) * p.Wn, 0x3333333333333333ull);
    if (!p.rg_kind.empty()) {   // feature level 3: generic reservations
        a.n_rg = (u32)p.rg_kind.size();
        a.gstride = N;
        a.gcnt = em.gcnt.data();
        a.rg = rg.data();
        a.tg = p.tg.data();
        a.gs_off = p.gs_off.data();
        a.gs_row = p.gs_row.data();
        a.rg_kind = p.rg_kind.data();
        a.rg_val = p.rg_val.data();
        a.rg_k0 = p.rg_k0.data();
        a.rg_k1 = p.rg_k1.data();
    }
    a.tmpl = nullptr;

    u64 rounds = 0;
    auto stretch = [&](u32 j0, u32 j1) -> bool {   // the block resolver over [j0, j1): bitmaps from the node rows as they are, then rounds
        grid(1, 1024, 256, [a]() { k_r6_minmax(a); });
        grid((p.Wn + 3) / 4, 256, 0, [a]() { k_r6_rows(a); });
        if (blk.error) { fprintf(stderr, "build reported error %u\n", blk.error); return false; }
        blk.pos = j0;
        blk.end = j1;
        while (blk.pos < blk.end) {
            const u32 before = blk.pos;
            for (R6Prop& q : prop) memset(&q, 0xEE, sizeof q);
            grid(B, 64 * R6_PW, r6_propose_lds(p.Wn), [a]() { k_r6_propose(a); });
            grid(1, R6_COMMIT_THREADS, r6_commit_lds(p.Wn, B, n_dc + n_dm), [a]() { k_r6_commit(a); });
            ++rounds;
            if (blk.error) { fprintf(stderr, "kernel reported error %u at task %u\n", blk.error, blk.pos); return false; }
            if (blk.pos <= before) { fprintf(stderr, "no progress at task %u\n", before); return false; }
        }
        return blk.pos == j1;
    };
    std::vector<u32> hmat((size_t)S * N, 0xABABABABu), emat((size_t)S * N, 0xCDCDCDCDu);
    guard("hmat", hmat);
    guard("emat", emat);
    u32 spread_error = 0;
    auto spread = [&](u32 j0, u32 j1) -> bool {
        SpreadArgs sp{};
        ScanArgs& s = sp.s;
        s.a = a;
        s.j0 = j0;
        s.j1 = j1;
        s.n_svc = S;
        s.n_sc = p.n_sc;
        s.hmat = hmat.data();
        s.emat = emat.data();
        sp.ttree = ttree.data();
        sp.tree_off = tree_off.data();
        sp.tn_parent = tn_parent.data();
        sp.tn_first = tn_first.data();
        sp.tn_next = tn_next.data();
        sp.tn_nchild = tn_nchild.data();
        sp.tn_depth = tn_depth.data();
        sp.leaf_of_node = leaf_of.data();
        sp.max_ntn = max_ntn;
        sp.max_depth = max_depth;
        sp.n_trees = (u32)tree_keys.size();
        sp.tot_ntn = tree_off.back();
        blk.error = 0;
        grid(1024, 256, 0, [s]() { k_scan_fill(s); });
        for (u32 sv = 0; sv < S; ++sv) {
            emu::blockidx_y() = sv;
            grid(64, 256, 0, [s]() { k_scan_lists(s); });
        }
        emu::blockidx_y() = 0;
        grid(1, SCAN_THREADS, scan_lds_spw(max_ntn, max_depth, sp.n_trees, sp.tot_ntn), [sp]() { k_scan_spread_wide(sp); });
        ++rounds;
        spread_error = blk.error;
        if (tot_bad) return true;   // (judged below)
        if (blk.error) { fprintf(stderr, "k_scan_spread_wide reported error %u\n", blk.error); return false; }
        return blk.pos == j1;
    };
    bool ok = mixed ? (stretch(0, T / 3) && spread(T / 3, 2 * T / 3) && stretch(2 * T / 3, T)) : spread(0, T);
    if (!ok) return 3;
    if (tot_bad) {   // the error, the position, and below: everything the tasks in front of it did
        if (spread_error != ERR_LEVEL_RANGE) { fprintf(stderr, "flag T: error %u, ERR_LEVEL_RANGE expected\n", spread_error); ok = false; }
        if (blk.pos != stop_at) { fprintf(stderr, "flag T: the segment stopped at task %u, the model says %u\n", blk.pos, stop_at); ok = false; }
        for (u32 j = stop_at; j < T; ++j)
            if (em.out[j] != -1) { fprintf(stderr, "flag T: task %u behind the stop was placed on %d\n", j, em.out[j]); ok = false; }
    }

    ok = ok && same("out", em.out, ref.out, T) && same("cpu", em.cpu, ref.cpu, N) && same("mem", em.mem, ref.mem, N) && same("total", em.total, ref.total, N) &&
         same("X", em.X, ref.X, em.X.size()) && same("portmap", em.portmap, ref.portmap, em.portmap.size()) &&
         same("list_node", em.list_node, ref.list_node, em.list_node.size()) && same("list_svc", em.list_svc, ref.list_svc, em.list_svc.size()) &&
         same("list_fail", em.list_fail, ref.list_fail, em.list_fail.size()) && same("gcnt", em.gcnt, ref.gcnt, em.gcnt.size());
    ok = ok && em.ctl.ncommit == ref.ctl.ncommit && em.ctl.ninf == ref.ctl.ninf;
    if (!ok) fprintf(stderr, "ncommit emu %u ref %u, ninf emu %u ref %u\n", em.ctl.ncommit, ref.ctl.ncommit, em.ctl.ninf, ref.ctl.ninf);
    ok = ok && same("log_node", em.log_node, ref.log_node, ref.ctl.ncommit) && same("log_task", em.log_task, ref.log_task, ref.ctl.ncommit) &&
         same("log_prev", em.log_prev, ref.log_prev, ref.ctl.ncommit) && same("last", em.last, ref.last, N) &&
         same("inf_task", em.inf_task, ref.inf_task, ref.ctl.ninf) && same("inf_pos", em.inf_pos, ref.inf_pos, ref.ctl.ninf);
    for (auto& chk : g_guards) ok = chk() && ok;
    u32 top_bit = 0, max_total = 0;
    for (u32 j = 0; j < T; ++j) top_bit += em.out[j] >= 32768;
    for (u32 n = 0; n < N; ++n) max_total = std::max(max_total, em.total[n]);
    if (ok && high && top_bit == 0) { fprintf(stderr, "flag h: no pick with the key's top node bit\n"); ok = false; }
    if (ok && tie && !(em.out[0] == (int32_t)tie_lo && em.out[1] == (int32_t)tie_hi)) { fprintf(stderr, "flags e / E: tasks 0 and 1 on nodes %d and %d, expected %u and %u\n", em.out[0], em.out[1], tie_lo, tie_hi); ok = false; }
    if (ok && dead && model.noroom_events == 0) { fprintf(stderr, "flag d: the walk met no branch without room\n"); ok = false; }
    if (ok && tot_ok && max_total < 65535) { fprintf(stderr, "flag t: no node holds 65 535 tasks\n"); ok = false; }
    (void)verbose;
    fprintf(stderr, "picks with the top node bit %u | largest task total of a node %u | stopped at task %u of %u with error %u | guard zones checked %zu\n", top_bit, max_total, tot_bad ? blk.pos : T, T, spread_error, g_guards.size());
    fprintf(stderr, "spread tasks placed %llu, left without a node %llu | branches found without room %llu | calls that handed a branch more than one task %llu | trees: largest %u nodes, deepest %u levels\n",
            (unsigned long long)model.spread_placed, (unsigned long long)model.spread_unplaced, (unsigned long long)model.noroom_events, (unsigned long long)model.handed_more, max_ntn, max_depth);
    fprintf(stderr, "seed %u N %u T %u S %u block %u order %d feat %d levels %u values %u: placed %u inf %u | launches %llu -> %s\n", seed, N, T, S, B, order, feat, levels, vals,
            em.ctl.ncommit, em.ctl.ninf, (unsigned long long)rounds, ok ? "OK" : "FAIL");
    return ok ? 0 : 1;
}
