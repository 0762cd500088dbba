// emu_groups_stream.cpp — the STREAMED instance of the task-group kernel (swarmkit_amd/csrc/swp_groups.hpp: k_groups2s, the machine's
// G2_OP_PUBLISH command, helper 0's publish) on CPU fibers, over the random problems and against the sequential model of
// emu_groups.cpp (included under another name for its main: problems, model and harness are that file's, not copies).
// What is checked: standing where the polling host stands — at every release store of the mark counter — the placements in front of
// the mark are the model's FINAL ones and no sentinel is left; the marks are the ones the host computes up front
// (swp_rounds.hpp group_marks); at the end every output and all mutated state equal the model's, as in emu_groups.cpp; the command
// ring never holds more than it has entries for (posted - min(helper position) <= G2_RING at every post); a cancel word set at a
// chosen mark ends the launch with ERR_GROUP_CANCELLED, without a hang, and what was published up to then is still the model's.
// TEST INFRASTRUCTURE (tests/test_emu_groups_stream.py); not product.
//
//   emu_groups_stream <seed> <N> <groups> <kmax> <trees> <features 0..3> <threads> <step> <cancel at mark, 0: never> [v] [u]
// Built twice by the test: as is, and with -DG2_ARENA_LDS=3072. EMU_SCHED_SEED: wv_emu.hpp's random wave schedules.
#include "wv_emu_sys.hpp"

// ---- the ring-occupancy assertion: the kernel's hooks (swp_groups.hpp G2_RING_CHECK, G2_HELPER_AT) ----
static unsigned g2s_read[64];      // per helper: commands read off the ring so far
static unsigned g2s_helpers = 0, g2s_max_occ = 0, g2s_posted = 0;
static bool g2s_ring_bad = false;
static void g2s_ring_check(unsigned posted);
#define G2_RING_CHECK(posted) g2s_ring_check(posted)
#define G2_HELPER_AT(hid, my) do { if (wv::lane() == 0) g2s_read[hid] = (my) + 1u; } while (0)
#define SWP_G2_STREAM

#define main emu_groups_plain_main
#include "emu_groups.cpp"
#undef main

#include "../../swarmkit_amd/csrc/swp_rounds.hpp"

static void g2s_ring_check(unsigned posted) {
    if (wv::lane() != 0) return;
    unsigned lo = ~0u;
    for (unsigned h = 0; h < g2s_helpers; ++h) lo = std::min(lo, g2s_read[h]);
    g2s_posted = posted;
    g2s_max_occ = std::max(g2s_max_occ, posted - lo);
    if (posted - lo > G2_RING) g2s_ring_bad = true;
}

static const int32_t SENTINEL = (int32_t)0x80000000;   // PUB_SENTINEL (swp_publish.hpp)

int main(int argc, char** argv) {
    if (argc < 10) { fprintf(stderr, "usage: %s seed N groups kmax trees features(0..3) threads step cancel_at [v] [u]\n", argv[0]); return 2; }
    const u32 seed = atoi(argv[1]), N = atoi(argv[2]), n_groups = atoi(argv[3]), kmax = atoi(argv[4]), n_trees = atoi(argv[5]);
    const int feat = atoi(argv[6]);
    const u32 threads = atoi(argv[7]), step_knob = atoi(argv[8]), cancel_at = atoi(argv[9]);
    bool verbose = false;
    for (int i = 10; i < argc; ++i) {
        if (argv[i][0] == 'v') verbose = true;
        if (argv[i][0] == 'u') g_level_start = true;
    }
    Problem p = make_problem(seed, N, n_groups, kmax, n_trees, feat);
    Model m(p);
    m.run();

    // ---- the kernel's inputs (as emu_groups.cpp's main lays them out) ----
    State em = p.st0;
    const u32 Wn = p.Wn;
    std::vector<u32> tree_off{0}, tn_parent, tn_first, tn_next, tn_nchild, tn_nodes, leaf_of;
    u32 max_ntn = 1, max_depth = 0;
    for (const Tree& t : p.trees) {
        tn_parent.insert(tn_parent.end(), t.parent.begin(), t.parent.end());
        tn_first.insert(tn_first.end(), t.first.begin(), t.first.end());
        tn_next.insert(tn_next.end(), t.next.begin(), t.next.end());
        tn_nchild.insert(tn_nchild.end(), t.nchild.begin(), t.nchild.end());
        tn_nodes.insert(tn_nodes.end(), t.nodes.begin(), t.nodes.end());
        leaf_of.insert(leaf_of.end(), t.leaf_of.begin(), t.leaf_of.end());
        tree_off.push_back((u32)tn_parent.size());
        max_ntn = std::max<u32>(max_ntn, (u32)t.parent.size());
        max_depth = std::max(max_depth, t.depth);
    }
    std::vector<u32> list_off(p.S + 1, 0), list_cnt(p.S, 0), list_node, list_svc, list_fail, svc_tasks(p.S, 0);
    for (const GroupRec2& g : p.groups) svc_tasks[g.svc] += g.k;
    for (u32 q = 0; q < p.S; ++q) {
        list_off[q] = (u32)list_node.size();
        for (auto& kv : p.st0.svc[q]) { list_node.push_back(kv.first); list_svc.push_back(kv.second.first); list_fail.push_back(kv.second.second); }
        list_cnt[q] = (u32)list_node.size() - list_off[q];
        list_node.insert(list_node.end(), svc_tasks[q], LIST_EMPTY);
        list_svc.insert(list_svc.end(), svc_tasks[q], 0u);
        list_fail.insert(list_fail.end(), svc_tasks[q], 0u);
    }
    list_off[p.S] = (u32)list_node.size();
    list_node.push_back(LIST_EMPTY); list_svc.push_back(0); list_fail.push_back(0);
    size_t arena_bytes = 64;
    u32 total_out = 0, special = 0, deps = 0;
    std::vector<u32> sizes;
    for (const GroupRec2& g : p.groups) {
        arena_bytes = std::max(arena_bytes, g2_arena_bytes(g.n_slots, tree_off[g.tree + 1] - tree_off[g.tree], g.n_gen, max_depth, g.k));
        total_out += g.k;
        sizes.push_back(g.k);
        special += (g.flags & RT_PORTS) || g.n_gen;   // the unfused write-back
        deps += g.dep_prev;                            // nothing evaluated ahead
    }
    std::vector<unsigned char> ffbuf((size_t)2 * N, 0xEE), arena(arena_bytes + 64, 0xCD);
    std::vector<u64> keybuf((size_t)2 * N, 0xEEEEEEEEEEEEEEEEull), xroot(max_ntn, 0);
    std::vector<u32> svc_dense((size_t)2 * N, 0), fail_dense((size_t)2 * N, 0), lpos_dense((size_t)2 * N, 0);
    std::vector<G2Cand> ccand((size_t)2 * N, G2Cand{0x3333, 0xEEEEEEEEu, 0xEEEEEEEEu});
    std::vector<u32> cpos((size_t)2 * N, 0xEEEEEEEEu);
    std::vector<u64> cmin((size_t)2 * Wn, 0x6666);
    std::vector<u32> scls_def;
    {
        std::map<std::tuple<u32, u32, u32>, u32> ids;
        for (GroupRec2& g : p.groups) {
            auto key = std::make_tuple(g.cls_plug, g.cls_con, g.cls_plat);
            auto it = ids.find(key);
            if (it == ids.end()) {
                it = ids.emplace(key, (u32)ids.size()).first;
                scls_def.push_back(g.cls_plug); scls_def.push_back(g.cls_con); scls_def.push_back(g.cls_plat);
            }
            g.scls = it->second;
        }
    }
    const u32 n_scls = (u32)scls_def.size() / 3;
    std::vector<u32> slist((size_t)n_scls * N, 0xEEEEEEEEu), scnt(n_scls, 0x7777);
    std::vector<u64> sbits((size_t)n_scls * Wn, 0x8888);
    std::vector<i64> tsumbuf((size_t)2 * max_ntn, 0x7777);
    std::vector<int32_t> xadm(max_ntn, 0), out(total_out, -7);
    std::vector<u32> hist(p.groups.size() * 8, 0);
    Ctl ctl;
    memset(&ctl, 0, sizeof ctl);
    Groups2Args a;
    memset(&a, 0, sizeof a);
    a.n_nodes = N; a.n_words = Wn; a.n_groups = (u32)p.groups.size(); a.gstride = N; a.max_ntn = max_ntn; a.max_depth = max_depth;
    a.g = p.groups.data();
    a.valid = p.valid.data(); a.ready = p.ready.data(); a.con = p.con.data(); a.plat = p.plat.data(); a.plug = p.plug.data();
    a.cpu = em.cpu.data(); a.mem = em.mem.data(); a.total = em.total.data(); a.gcnt = em.gcnt.data();
    a.portmap = em.portmap.data(); a.pset_off = p.pset_off.data(); a.pset_ids = p.pset_ids.data();
    a.list_node = list_node.data(); a.list_svc = list_svc.data(); a.list_fail = list_fail.data(); a.list_off = list_off.data(); a.list_cnt = list_cnt.data();
    a.tree_off = tree_off.data(); a.tn_parent = tn_parent.data(); a.tn_first = tn_first.data(); a.tn_next = tn_next.data();
    a.tn_nchild = tn_nchild.data(); a.tn_nodes = tn_nodes.data(); a.leaf_of_node = leaf_of.data();
    a.ffbuf = ffbuf.data(); a.keybuf = keybuf.data(); a.ccand = ccand.data(); a.cpos = cpos.data(); a.cmin = cmin.data();
    a.n_scls = n_scls; a.scls_def = scls_def.data(); a.slist = slist.data(); a.scnt = scnt.data(); a.sbits = sbits.data();
    a.svc_dense = svc_dense.data(); a.fail_dense = fail_dense.data(); a.lpos_dense = lpos_dense.data();
    a.tsumbuf = tsumbuf.data(); a.xroot = xroot.data(); a.xadm = xadm.data(); a.arena = arena.data();
    a.out_node = out.data(); a.hist = hist.data(); a.ctl = &ctl;
    for (u32 c = 0; c < n_scls; ++c) {
        emu::blockidx() = c;
        emu::launch(64, 0, [&] { k_g2_static(a); });
    }
    emu::blockidx() = 0;

    // ---- the host-visible block, and the host's place at the counter ----
    const u32 step = group_pub_step(total_out, (u32)sizes.size(), step_knob);
    std::vector<u32> want_marks;
    const u32 n_marks = group_marks(sizes.data(), (u32)sizes.size(), step, [&](uint32_t mark, uint32_t) { want_marks.push_back(mark); });
    std::vector<int32_t> h_pub(total_out, SENTINEL);
    std::vector<u32> h_ring(StreamMarks::RING, 0xABABABABu), got_marks;
    u32 h_count = 0, h_cancel = 0, d_stop = 0xFFFFFFFFu;
    G2Pub pb;
    pb.h_pub = h_pub.data(); pb.h_ring = h_ring.data(); pb.h_count = &h_count; pb.h_cancel = &h_cancel; pb.d_stop = &d_stop;
    pb.step = step; pb.ring = StreamMarks::RING;
    int bad = 0;
    auto fail = [&](const char* what, size_t i, long long x, long long y) {
        if (bad++ < 12) fprintf(stderr, "MISMATCH %s[%zu]: kernel %lld, model %lld\n", what, i, x, y);
    };
    emu::sys_release_hook() = [&](const u32* word, u32 v) {
        if (word != &h_count) { fail("release store to a word that is not the counter", 0, 0, 0); return; }
        if (v != (u32)got_marks.size() + 1u) fail("mark counter", got_marks.size(), v, (long long)got_marks.size() + 1);
        const u32 mark = h_ring[(v - 1u) % StreamMarks::RING];
        if (mark > total_out || (!got_marks.empty() && mark <= got_marks.back())) { fail("mark", v - 1u, mark, total_out); return; }
        got_marks.push_back(mark);
        for (u32 i = 0; i < mark; ++i) {   // the whole prefix, every time: nothing in front of a mark may move again
            if (h_pub[i] == SENTINEL) fail("published prefix holds a sentinel", i, h_pub[i], m.out[i]);
            else if (h_pub[i] != m.out[i]) fail("published prefix", i, h_pub[i], m.out[i]);
        }
        if (cancel_at && v == cancel_at) h_cancel = 1u;
    };
    g2s_helpers = threads / 64u - 1u;
    emu::launch(threads, g2_lds_bytes(), [&] { k_groups2s(a, pb); });
    emu::sys_release_hook() = nullptr;

    // ---- compare ----
    if (g2s_ring_bad) fail("command ring: posted - min(helper position)", 0, g2s_max_occ, G2_RING);
    if (cancel_at) {
        if (cancel_at > n_marks) { fprintf(stderr, "cancel_at %u beyond the tick's %u marks\n", cancel_at, n_marks); return 2; }
        if (ctl.error != ERR_GROUP_CANCELLED) fail("ctl.error after a cancel", 0, ctl.error, ERR_GROUP_CANCELLED);
        if (d_stop > p.groups.size()) fail("stop word", 0, d_stop, (long long)p.groups.size());
        if (got_marks.size() < cancel_at || got_marks.size() > want_marks.size() || !std::equal(got_marks.begin(), got_marks.end(), want_marks.begin()))
            fail("marks before the cancel are not a prefix of the host's", 0, (long long)got_marks.size(), (long long)want_marks.size());
        // the machine looks at the error word at a group's start: it may finish groups posted meanwhile, never run past the end unnoticed
        const u32 stop_end = d_stop ? p.groups[d_stop - 1].out_off + p.groups[d_stop - 1].k : 0u;
        if (!got_marks.empty() && got_marks.back() > stop_end) fail("a mark beyond the groups the machine went through", 0, got_marks.back(), stop_end);
        for (u32 i = 0; i < stop_end; ++i)
            if (out[i] != m.out[i]) fail("out_node in front of the stop", i, out[i], m.out[i]);
        if (verbose || bad)
            fprintf(stderr, "emu_groups_stream seed %u N %u groups %zu step %u: cancelled at mark %u of %u, %zu marks seen, stopped after group %u, ring occupancy at most %u -> %s\n", seed, N,
                    p.groups.size(), step, cancel_at, n_marks, got_marks.size(), d_stop, g2s_max_occ, bad ? "FAILED" : "OK");
        return bad ? 1 : 0;
    }
    if (ctl.error != ERR_NONE) { fprintf(stderr, "kernel reported error %u\n", ctl.error); return 1; }
    if (got_marks != want_marks) fail("marks differ from the host's rule", 0, (long long)got_marks.size(), (long long)want_marks.size());
    if (h_count != n_marks) fail("mark counter at the end", 0, h_count, n_marks);
    if (d_stop != p.groups.size()) fail("stop word", 0, d_stop, (long long)p.groups.size());
    for (size_t i = 0; i < out.size(); ++i) {
        if (out[i] != m.out[i]) fail("out_node", i, out[i], m.out[i]);
        if (h_pub[i] != m.out[i]) fail("h_pub", i, h_pub[i], m.out[i]);
    }
    for (size_t i = 0; i < hist.size(); ++i)
        if (hist[i] != m.hist[i]) fail("hist", i, hist[i], m.hist[i]);
    for (u32 n = 0; n < N; ++n) {
        if (em.cpu[n] != m.s.cpu[n]) fail("cpu", n, em.cpu[n], m.s.cpu[n]);
        if (em.mem[n] != m.s.mem[n]) fail("mem", n, em.mem[n], m.s.mem[n]);
        if (em.total[n] != m.s.total[n]) fail("total", n, em.total[n], m.s.total[n]);
    }
    for (size_t i = 0; i < em.gcnt.size(); ++i)
        if (em.gcnt[i] != m.s.gcnt[i]) fail("gcnt", i, em.gcnt[i], m.s.gcnt[i]);
    for (size_t i = 0; i < em.portmap.size(); ++i)
        if (em.portmap[i] != m.s.portmap[i]) fail("portmap", i, (long long)em.portmap[i], (long long)m.s.portmap[i]);
    for (u32 q = 0; q < p.S; ++q) {
        std::map<u32, std::pair<u32, u32>> got;
        for (u32 e = list_off[q]; e < list_off[q] + list_cnt[q]; ++e) {
            if (list_node[e] == LIST_EMPTY) { fail("list hole", e, 0, 0); continue; }
            if (got.count(list_node[e])) fail("list duplicate", e, list_node[e], 0);
            got[list_node[e]] = {list_svc[e], list_fail[e]};
        }
        if (got != m.s.svc[q]) fail("service list", q, (long long)got.size(), (long long)m.s.svc[q].size());
    }
    for (size_t i = 0; i < svc_dense.size(); ++i)
        if (svc_dense[i] || fail_dense[i] || lpos_dense[i]) { fail("dense column not cleared", i, svc_dense[i], 0); break; }
    u32 lds_groups = 0;
    for (const GroupRec2& g : p.groups) lds_groups += g2_arena_bytes(g.n_slots, tree_off[g.tree + 1] - tree_off[g.tree], g.n_gen, max_depth, g.k) <= G2_ARENA_LDS;
    if (verbose || bad)
        fprintf(stderr, "emu_groups_stream seed %u N %u groups %zu (LDS arena: %u, same service as the one before: %u, ports or generic: %u) %u tasks, step %u: %u marks, %u commands posted, ring occupancy at most %u of %u -> %s\n",
                seed, N, p.groups.size(), lds_groups, deps, special, total_out, step, n_marks, g2s_posted, g2s_max_occ, G2_RING, bad ? "FAILED" : "OK");
    return bad ? 1 : 0;
}
