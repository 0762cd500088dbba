// emu_scan_spread_compact.cpp — runs the COMPACT spread instance of the scan resolver (swarmkit_amd/csrc/swp_scan_spread.hpp:
// k_scan_spread<.., true> behind the probe k_scan_mark + k_scan_union, the compact matrices k_scan_fill_c / k_scan_lists_c and the base
// sums k_spread_base) on CPU fibers, on a nodeSet of more than SCAN_MAXN nodes of which Nc — a pool scattered over the index range — pass
// the class rows of the segment's tasks, against the sequential model of emu_scan_spread.cpp (written from the reference's text:
// nodeSet.tree with a heap of one over ALL nodes of the nodeSet, scheduleNTasksOnSubtree as the recursion it is, NodeInfo.addTask) —
// every output, every mutated array. TEST INFRASTRUCTURE (tests/test_emu_scan_spread_compact.py); not product.
//
//   emu_scan_spread_compact <seed> <N> <T> <S> <block> <order: 0 rr | 1 major | 2 random> <features 0..3> <levels 0..3> <values per key 1..> <Nc 0..4096> [flags]
//   flags: v verbose | m block / spread / block in thirds: the outer thirds' tasks carry no preferences and name class rows over ALL
//   nodes, so the block resolver places tasks of the segment's services outside the segment's union | l a fifth of the nodes lack each
//   label (the "" branch) | o nodes OUTSIDE the union whose first label has value 2 carry tasks of every service (a leaf that also holds
//   union nodes starts from a base sum; asserted: a base sum is non-zero, and the model's placements differ from those of the model
//   run with the outside counts removed) | d the nodes whose first label has value 1 are all outside the union and two of them carry a
//   task of every service (a first-level branch the walk finds without room)
#include "wv_emu.hpp"

#define SWP_R6_KERNELS
#include "../../swarmkit_amd/csrc/swp_resolve6.hpp"
#define SWP_SCAN_KERNELS          // (k_scan_fill, k_scan_lists: the matrices)
#define SWP_SCAN_SPREAD_KERNEL
#include "../../swarmkit_amd/csrc/swp_scan_spread.hpp"

#include "emu_model.hpp"

template <class F>
static void grid(u32 blocks, u32 threads, size_t lds, F body) {
    for (u32 b = 0; b < blocks; ++b) {
        emu::blockidx() = b;
        emu::launch(threads, lds, body);
    }
    emu::blockidx() = 0;
}

// ---- the model ----------------------------------------------------------------------------------------------------------------
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

int main(int argc, char** argv) {
    if (argc < 11) { fprintf(stderr, "usage: %s seed N T S block order features(0..3) levels(0..3) values Nc [v] [m] [d] [l] [o]\n", argv[0]); return 2; }
    const u32 seed = atoi(argv[1]);
    u32 N = atoi(argv[2]), T = atoi(argv[3]), S = atoi(argv[4]);
    const u32 B = atoi(argv[5]);
    const int order = atoi(argv[6]), feat = atoi(argv[7]);
    const u32 levels = std::min(3, atoi(argv[8])), vals = std::max(1, atoi(argv[9]));
    const u32 Nc = atoi(argv[10]);
    bool verbose = false, mixed = false, dead = false, lack = false, outside = false;
    for (int i = 11; i < argc; ++i) {
        if (argv[i][0] == 'v') verbose = true;
        if (argv[i][0] == 'm') mixed = true;
        if (argv[i][0] == 'd') dead = true;
        if (argv[i][0] == 'l') lack = true;
        if (argv[i][0] == 'o') outside = true;
    }
    if (N <= SCAN_MAXN || Nc > SCAN_MAXN) { fprintf(stderr, "more than %d nodes, of which at most %d in the union\n", SCAN_MAXN, SCAN_MAXN); return 2; }
    if ((dead || outside) && (levels == 0 || vals < 3)) { fprintf(stderr, "flags d and o need a level and three values\n"); return 2; }
    Problem p = make_problem(seed, N, T, S, order, feat);
    // labels and trees: a generator of their own (make_problem's stream is not touched)
    std::mt19937_64 g(0xA0761D6478BD642Full * (seed + 1) + 0x5B);
    auto rnd = [&](u32 k) { return (u32)(g() % k); };
    std::vector<std::vector<u32>> label(3, std::vector<u32>(N, 0));
    for (u32 k = 0; k < 3; ++k)
        for (u32 n = 0; n < N; ++n) label[k][n] = (lack && rnd(5) == 0) ? 0u : 1 + rnd(vals);
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
    // The union: exactly Nc nodes, scattered — the last node first, then the first and the last bit of words, then random ones (d: none
    // whose first label is 1). They are all valid; class row 0 is exactly this set, every other row of the first 22 what it was inside
    // it. Service 0 asks for row 0, so a segment with a task of it has all Nc nodes in its union. Rows 22 .. 43 are the rows as
    // make_problem left them, over all nodes: what the outer thirds of `m` name.
    std::vector<u64> E(p.Wn, 0);
    {
        u32 have = 0, tries = 0;
        auto take = [&](u32 n) {
            if (have == Nc || n >= N || ((E[n >> 6] >> (n & 63)) & 1) || (dead && label[0][n] == 1)) return;
            E[n >> 6] |= 1ull << (n & 63);
            ++have;
        };
        take(N - 1);
        const u32 edge[] = {63, 64, 127, 4095, 4096, (p.Wn - 1) * 64, (p.Wn - 1) * 64 - 1, 0};
        for (u32 n : edge) take(n);
        while (have < Nc && ++tries < 100u * N) take(rnd(N));
        if (have != Nc) { fprintf(stderr, "no %u nodes for the union\n", Nc); return 2; }
    }
    auto in_union = [&](u32 n) { return ((E[n >> 6] >> (n & 63)) & 1) != 0; };
    for (u32 w = 0; w < p.Wn; ++w) p.valid[w] |= E[w];
    {
        std::vector<u64> all = p.sc;
        p.sc.resize((size_t)2 * p.n_sc * p.Wn);
        for (u32 c = 0; c < p.n_sc; ++c)
            for (u32 w = 0; w < p.Wn; ++w) {
                p.sc[(size_t)(p.n_sc + c) * p.Wn + w] = all[(size_t)c * p.Wn + w];
                p.sc[(size_t)c * p.Wn + w] = c == 0 ? E[w] : all[(size_t)c * p.Wn + w] & E[w];
            }
        for (u32 j = 0; j < T; ++j) {
            if (p.rt[j].svc == 0) p.rt[j].sc = 0;
            if (mixed && (j < T / 3 || j >= 2 * T / 3)) p.rt[j].sc += p.n_sc;
        }
        p.n_sc *= 2;
    }
    // the lists laid out again with the flags' entries on nodes outside the union (make_problem's own entries lie anywhere)
    std::vector<std::pair<u32, u32>> extra;   // (node, count) for EVERY service
    if (outside) {
        u32 have = 0;
        for (u32 n = 0; n < N && have < 24; ++n)
            if (!in_union(n) && ((p.valid[n >> 6] >> (n & 63)) & 1) && label[0][n] == 2) { extra.push_back({n, 1 + rnd(4)}); ++have; }
        if (have < 8) { fprintf(stderr, "flag o: too few nodes outside the union in branch 2\n"); return 2; }
    }
    if (dead) {
        u32 have = 0;
        for (u32 n = N; n-- > 0 && have < 2;)
            if (((p.valid[n >> 6] >> (n & 63)) & 1) && label[0][n] == 1) { extra.push_back({n, 1}); ++have; }
        if (have < 2) { fprintf(stderr, "flag d: no nodes in branch 1\n"); return 2; }
    }
    if (!extra.empty()) {
        std::vector<u32> ln, ls, lf, off(S + 1, 0), init(S, 0), rank(T), seen(S, 0);
        for (u32 j = 0; j < T; ++j) rank[j] = seen[p.rt[j].svc]++;
        std::fill(p.X.begin(), p.X.end(), 0ull);
        for (u32 s = 0; s < S; ++s) {
            off[s] = (u32)ln.size();
            std::set<u32> had;
            for (u32 e = p.list_off[s]; e < p.list_off[s + 1]; ++e)
                if (p.list_node[e] != LIST_EMPTY) { ln.push_back(p.list_node[e]); ls.push_back(p.list_svc[e]); lf.push_back(p.list_fail[e]); had.insert(p.list_node[e]); }
            for (auto& x : extra)
                if (!had.count(x.first)) { ln.push_back(x.first); ls.push_back(x.second); lf.push_back(0); }
            init[s] = (u32)ln.size() - off[s];
            for (u32 e = off[s]; e < ln.size(); ++e) p.X[(size_t)s * p.Wn + (ln[e] >> 6)] |= 1ull << (ln[e] & 63);
            for (u32 i = 0; i < seen[s]; ++i) { ln.push_back(LIST_EMPTY); ls.push_back(0); lf.push_back(0); }
        }
        off[S] = (u32)ln.size();
        p.list_off = off; p.list_node = ln; p.list_svc = ls; p.list_fail = lf;
        for (u32 j = 0; j < T; ++j) p.rt[j].slot = off[p.rt[j].svc] + init[p.rt[j].svc] + rank[j];
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
    Model model(p, ref, label, tree_keys);
    for (u32 j = 0; j < T; ++j) model.task(j, ttree[j]);
    // flag o: the model again with the counts of the nodes outside the union removed — what a compaction without base sums computes
    u32 differ = 0;
    if (outside) {
        Problem q = p;
        for (u32 e = 0; e < q.list_node.size(); ++e)
            if (q.list_node[e] != LIST_EMPTY && !in_union(q.list_node[e])) q.list_svc[e] = 0;
        State alt = initial_state(q);
        Model m2(q, alt, label, tree_keys);
        for (u32 j = 0; j < T; ++j) m2.task(j, ttree[j]);
        for (u32 j = 0; j < T; ++j) differ += alt.out[j] != ref.out[j];
    }
    // the (service, tree) pairs, in the order their first task appears (the engine's build_batch)
    std::vector<u32> tpair(T), pair_svc, pair_tree;
    {
        std::map<std::pair<u32, u32>, u32> local;
        for (u32 j = 0; j < T; ++j) {
            auto k = std::make_pair(p.rt[j].svc, ttree[j]);
            auto it = local.find(k);
            if (it == local.end()) { it = local.emplace(k, (u32)pair_svc.size()).first; pair_svc.push_back(k.first); pair_tree.push_back(k.second); }
            tpair[j] = it->second;
        }
    }

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
    if (scan_lds_sp(Nc, max_ntn, max_depth, (u32)tree_keys.size(), tree_off.back()) > (size_t)160 * 1024 - 512) { fprintf(stderr, "the trees do not fit the LDS budget\n"); return 2; }

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
    std::vector<u32> hmat((size_t)S * std::max(Nc, 1u), 0xABABABABu), emat((size_t)S * std::max(Nc, 1u), 0xCDCDCDCDu);
    std::vector<u32> cused(p.n_sc, 0xEEEEEEEEu), cpre(p.Wn, 0xEEEEEEEEu), cmap(SCAN_MAXN, 0xEEEEEEEEu), base((size_t)pair_svc.size() * max_ntn, 0xEEEEEEEEu);
    std::vector<u64> cu(p.Wn, 0xEEEEEEEEEEEEEEEEull);
    u32 probe_nc = 0xEEEEEEEEu, base_nonzero = 0, segments = 0, rounds_outside = 0;
    bool probe_ok = true;
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
        s.cused = cused.data();
        s.cu = cu.data();
        s.cpre = cpre.data();
        s.cmap = cmap.data();
        s.cnc = &probe_nc;
        sp.tpair = tpair.data();
        sp.base = base.data();
        sp.n_pairs = (u32)pair_svc.size();
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
        // ---- the probe: the class rows the segment names, their union, its prefix sums and the map
        std::fill(cused.begin(), cused.end(), 0u);
        grid(std::min<u32>(64u, (j1 - j0 + 255u) / 256u), 256, 0, [s]() { k_scan_mark(s); });
        grid(1, SCAN_THREADS, scan_union_lds(), [s]() { k_scan_union(s); });
        {
            std::vector<u64> want(p.Wn, 0);
            for (u32 j = j0; j < j1; ++j)
                for (u32 w = 0; w < p.Wn; ++w) want[w] |= p.sc[(size_t)p.rt[j].sc * p.Wn + w];
            u32 cnt = 0;
            for (u32 w = 0; w < p.Wn; ++w) {
                if (cu[w] != want[w]) { fprintf(stderr, "probe: union word %u differs\n", w); probe_ok = false; }
                cnt += (u32)__builtin_popcountll(want[w]);
            }
            if (probe_nc != cnt) { fprintf(stderr, "probe: %u nodes counted, the union has %u\n", probe_nc, cnt); probe_ok = false; }
            if (probe_nc > SCAN_MAXN) { fprintf(stderr, "probe: the union has %u nodes\n", probe_nc); return false; }
            for (u32 c = 0; c < probe_nc; ++c) {
                const u32 n = cmap[c];
                if (n >= N || !((cu[n >> 6] >> (n & 63)) & 1) || (c && cmap[c - 1] >= n)) { fprintf(stderr, "probe: map[%u] = %u is not ascending inside the union\n", c, n); probe_ok = false; }
            }
        }
        s.n_c = probe_nc;
        sp.s.n_c = probe_nc;
        // ---- the compact matrices, the pairs' base sums from the lists as they are NOW, the kernel
        std::fill(hmat.begin(), hmat.end(), 0xABABABABu);
        std::fill(emat.begin(), emat.end(), 0xCDCDCDCDu);
        grid(1024, 256, 0, [s]() { k_scan_fill_c(s); });
        for (u32 sv = 0; sv < S; ++sv) {
            emu::blockidx_y() = sv;
            grid(64, 256, 0, [s]() { k_scan_lists_c(s); });
        }
        std::fill(base.begin(), base.end(), 0u);
        for (u32 pr = 0; pr < sp.n_pairs; ++pr) {
            emu::blockidx_y() = pr;
            const u32* ps = pair_svc.data();
            const u32* pt = pair_tree.data();
            u32* bs = base.data();
            grid(64, 256, 0, [sp, ps, pt, bs]() { k_spread_base(sp, ps, pt, bs); });
        }
        emu::blockidx_y() = 0;
        {   // the base sums against the lists: per pair with levels, per leaf, the counts of the entries outside the union
            std::vector<u32> want(base.size(), 0);
            for (u32 pr = 0; pr < sp.n_pairs; ++pr) {
                if (pair_tree[pr] == 0) continue;
                for (u32 e = p.list_off[pair_svc[pr]]; e < p.list_off[pair_svc[pr] + 1]; ++e) {
                    const u32 n = em.list_node[e];
                    if (n == LIST_EMPTY || ((cu[n >> 6] >> (n & 63)) & 1)) continue;
                    const u32 lf = leaf_of[(size_t)pair_tree[pr] * N + n];
                    if (lf != 0xFFFFFFFFu) want[(size_t)pr * max_ntn + lf] += em.list_svc[e];
                }
            }
            for (size_t i = 0; i < base.size(); ++i) {
                if (base[i] != want[i]) { fprintf(stderr, "base sum %zu: %u, the lists say %u\n", i, base[i], want[i]); probe_ok = false; }
                if (base[i]) ++base_nonzero;
            }
        }
        for (u32 e = 0; e < em.list_node.size(); ++e)   // entries the rounds in front made on nodes outside this segment's union
            if (p.list_node[e] == LIST_EMPTY && em.list_node[e] != LIST_EMPTY && !((cu[em.list_node[e] >> 6] >> (em.list_node[e] & 63)) & 1)) ++rounds_outside;
        ++segments;
        const size_t lds = scan_lds_sp(probe_nc, max_ntn, max_depth, sp.n_trees, sp.tot_ntn);
        switch (scan_nq(probe_nc)) {   // the instance the launcher picks for this union
            case 1: grid(1, SCAN_THREADS, lds, [sp]() { k_scan_spread<1, true>(sp); }); break;
            case 2: grid(1, SCAN_THREADS, lds, [sp]() { k_scan_spread<2, true>(sp); }); break;
            default: grid(1, SCAN_THREADS, lds, [sp]() { k_scan_spread<4, true>(sp); }); break;
        }
        ++rounds;
        if (blk.error) { fprintf(stderr, "k_scan_spread reported error %u\n", blk.error); return false; }
        return blk.pos == j1;
    };
    bool ok = mixed ? (stretch(0, T / 3) && spread(T / 3, 2 * T / 3) && stretch(2 * T / 3, T)) : spread(0, T);
    if (!ok) return 3;

    ok = ok && same("out", em.out, ref.out, T) && same("cpu", em.cpu, ref.cpu, N) && same("mem", em.mem, ref.mem, N) && same("total", em.total, ref.total, N) &&
         same("X", em.X, ref.X, em.X.size()) && same("portmap", em.portmap, ref.portmap, em.portmap.size()) &&
         same("list_node", em.list_node, ref.list_node, em.list_node.size()) && same("list_svc", em.list_svc, ref.list_svc, em.list_svc.size()) &&
         same("list_fail", em.list_fail, ref.list_fail, em.list_fail.size()) && same("gcnt", em.gcnt, ref.gcnt, em.gcnt.size());
    ok = ok && em.ctl.ncommit == ref.ctl.ncommit && em.ctl.ninf == ref.ctl.ninf;
    if (!ok) fprintf(stderr, "ncommit emu %u ref %u, ninf emu %u ref %u\n", em.ctl.ncommit, ref.ctl.ncommit, em.ctl.ninf, ref.ctl.ninf);
    ok = ok && same("log_node", em.log_node, ref.log_node, ref.ctl.ncommit) && same("log_task", em.log_task, ref.log_task, ref.ctl.ncommit) &&
         same("log_prev", em.log_prev, ref.log_prev, ref.ctl.ncommit) && same("last", em.last, ref.last, N) &&
         same("inf_task", em.inf_task, ref.inf_task, ref.ctl.ninf) && same("inf_pos", em.inf_pos, ref.inf_pos, ref.ctl.ninf);
    ok = ok && probe_ok;
    if (ok && outside && base_nonzero == 0) { fprintf(stderr, "flag o: every base sum is zero\n"); ok = false; }
    if (ok && outside && differ == 0) { fprintf(stderr, "flag o: the model places every task as it does without the outside counts: the case does not test the base sums\n"); ok = false; }
    if (ok && mixed && rounds_outside == 0) { fprintf(stderr, "flag m: the rounds in front of the segment placed no task outside its union\n"); ok = false; }
    if (ok && dead && model.noroom_events == 0) { fprintf(stderr, "flag d: the walk met no branch without room\n"); ok = false; }
    fprintf(stderr, "union of %u nodes (asked for %u) in %u segment(s) | non-zero base sums %u | placements that differ without the outside counts %u | list entries the rounds in front made outside the union %u\n", probe_nc, Nc, segments, base_nonzero, differ, rounds_outside);
    (void)verbose;
    fprintf(stderr, "spread tasks placed %llu, left without a node %llu | branches found without room %llu | calls that handed a branch more than one task %llu | trees: largest %u nodes, deepest %u levels\n",
            (unsigned long long)model.spread_placed, (unsigned long long)model.spread_unplaced, (unsigned long long)model.noroom_events, (unsigned long long)model.handed_more, max_ntn, max_depth);
    fprintf(stderr, "seed %u N %u T %u S %u block %u order %d feat %d levels %u values %u union %u: placed %u inf %u | launches %llu -> %s\n", seed, N, T, S, B, order, feat, levels, vals, Nc,
            em.ctl.ncommit, em.ctl.ninf, (unsigned long long)rounds, ok ? "OK" : "FAIL");
    return ok ? 0 : 1;
}
