// emu_volumes.cpp — runs the CSI volume code of swarmkit_amd/csrc/swp_volumes.hpp (vol_check, vol_for_mount, vol_filter_word, vol_choose,
// vol_reserve, k_vol_choose, k_vol_topology) and the preassigned pair pass (swp_fitpairs.hpp: k_fit_pairs_vol, k_fit_pairs) on CPU
// fibers (wv_emu.hpp) against the volume model of emu_model.hpp — a per-node, per-mount restatement of the reference's VolumeSet that keeps
// usage as the set of (task, node, read-only) and derives the device's numbers from it. TEST INFRASTRUCTURE (tests/test_emu_volumes.py).
//
//   emu_volumes selftest                          the MODEL against the known answers of tests/kat_volumes.py (checkVolume, IsInTopology)
//   emu_volumes functions <seed> <N>              k_vol_choose per (mount set, node), vol_filter_word per (set, word), vol_reserve over placements
//   emu_volumes topology <seed> <N>               k_vol_topology over its grid, two launches (vol0 > 0 for the second)
//   emu_volumes fitpairs <seed> <n_seg> <hot> [z] k_fit_pairs_vol against a sequential loop over the pairs; hot: pairs of segment 0; z: no volumes
//   emu_volumes fitpairs <seed> <n_seg> <hot> p   plain: no template has a mount set, the kernel is k_fit_pairs; no attachment row may be touched
// Every mode prints "reach ..." lines: what the MODEL's run came across (the Python test asserts on them), then "-> OK" or the difference.
#include "wv_emu.hpp"

#define SWP_VOL_KERNELS
#include "../../swarmkit_amd/csrc/swp_fitpairs.hpp"

#include <string>

#include "emu_model.hpp"

template <class F>
static void grid2(u32 bx, u32 by, u32 threads, F body) {
    for (u32 y = 0; y < by; ++y)
        for (u32 b = 0; b < bx; ++b) {
            emu::blockidx() = b;
            emu::blockidx_y() = y;
            emu::launch(threads, 0, body);
        }
    emu::blockidx() = 0;
    emu::blockidx_y() = 0;
}

static void print_reach(const char* mode, const VolReach& r) {
    fprintf(stderr, "reach %s:", mode);
    static const char* sh[4] = {"none", "readonly", "onewriter", "all"};
    for (u32 s = 0; s < 4; ++s) fprintf(stderr, " %s_rw=%llu %s_ro=%llu", sh[s], (unsigned long long)r.check[s][0], sh[s], (unsigned long long)r.check[s][1]);
    fprintf(stderr, " single_here=%llu single_elsewhere=%llu pin_many=%llu fail_first=%llu fail_later=%llu choice_ok=%llu refused_by_own=%llu\n", (unsigned long long)r.single_here,
            (unsigned long long)r.single_elsewhere, (unsigned long long)r.pin_many, (unsigned long long)r.fail_first, (unsigned long long)r.fail_later, (unsigned long long)r.choice_ok,
            (unsigned long long)r.refused_by_own);
}

static bool same_dyn(const VolProblem& vp, const VolUsage& use, const std::vector<VolDyn>& dev, const char* when, u64 step) {
    for (u32 v = 0; v < vp.vol.size(); ++v) {
        const VolDyn want = vp.derive(use, v);
        const VolDyn& d = dev[v];
        if (d.n_tasks != want.n_tasks || d.n_writers != want.n_writers || (want.n_tasks && d.pin != want.pin)) {
            fprintf(stderr, "MISMATCH usage of volume %u %s %llu: emu {%u tasks, %u writers, pin %08x} model {%u, %u, %08x}\n", v, when, (unsigned long long)step, d.n_tasks, d.n_writers, d.pin,
                    want.n_tasks, want.n_writers, want.pin);
            return false;
        }
    }
    return true;
}

// ---- selftest: the model against the project's own known answers (tests/kat_volumes.py CHECK_VOLUME and TOPOLOGY, stated in ids) ----
static int selftest() {
    bool ok = true;
    // checkVolume: plugin 1, subdomain 1 ("zone"), segments z1 = 1, z2 = 2; node 0 = someNode, node 1 = someOtherNode
    enum { UNUSED, WRONG_NODE, ONLY_READERS, WRITER };
    struct Row { const char* name; int multi, sharing, in_use; bool in_topology, ro, expected; };
    const Row rows[] = {
        {"volume outside of node topology", 0, MV_SH_ALL, UNUSED, false, false, false},
        {"volume in use on a different node", 0, MV_SH_ALL, WRONG_NODE, true, false, false},
        {"volume is read only, mount is not", 1, MV_SH_READ_ONLY, UNUSED, true, false, false},
        {"volume is OneWriter, but already has a writer", 1, MV_SH_ONE_WRITER, WRITER, true, false, false},
        {"volume is OneWriter, and has no writer", 1, MV_SH_ONE_WRITER, ONLY_READERS, true, false, true},
        {"volume not in use and is in topology", 0, MV_SH_ALL, UNUSED, true, false, true},
        {"in use on a different node, but the scope is multinode", 1, MV_SH_ALL, WRONG_NODE, true, false, true},
        {"the volume is in use and cannot be shared", 0, MV_SH_NONE, ONLY_READERS, true, true, false},
        {"the volume is not in use and cannot be shared", 0, MV_SH_NONE, UNUSED, true, true, true},
    };
    for (const Row& r : rows) {
        VolProblem vp;
        vp.N = 2;
        vp.node_csi.resize(2);
        MCsiInfo c;
        c.plugin = 1;
        c.has_topology = true;
        c.segments = {{1, r.in_topology ? 1u : 2u}};
        vp.node_csi[0].push_back(c);
        MVolume m;
        m.multi = r.multi != 0;
        m.sharing = (u32)r.sharing;
        m.driver = 1;
        m.accessible = {{{1, 1}}};
        vp.vol.push_back(m);
        VolUsage use(1);
        if (r.in_use == WRONG_NODE) use[0][1] = MUsage{1, false};
        if (r.in_use == ONLY_READERS || r.in_use == WRITER) use[0][1] = MUsage{0, true};
        if (r.in_use == WRITER) use[0][2] = MUsage{0, false};
        const bool got = vp.check_volume(use, 0, 0, r.ro);
        if (got != r.expected) { fprintf(stderr, "selftest checkVolume \"%s\": model %d, known answer %d\n", r.name, (int)got, (int)r.expected); ok = false; }
        // ... and the device function on the same row, through the tables
        vp.use0 = use;
        VolTables tb = vol_tables(vp);
        const VolView view = tb.view();
        if (vol_check(view, 0, 0, r.ro, nullptr) != r.expected) { fprintf(stderr, "selftest checkVolume \"%s\": vol_check differs from the known answer\n", r.name); ok = false; }
    }
    // IsInTopology: subdomains region 1, zone 2, shelf 3; segments R1 1, R2 2, Z1 3, Z2 4, Z3 5, S1 6, S2 7
    typedef std::vector<std::pair<u32, u32>> Seg;
    struct TRow { bool has_top; Seg top; std::vector<Seg> accessible; bool expected; };
    const TRow trows[] = {
        {true, {{1, 1}, {2, 3}}, {{{1, 1}, {2, 3}}}, true},
        {true, {{1, 1}, {2, 4}}, {{{1, 1}, {2, 3}}, {{1, 1}, {2, 4}}}, true},
        {true, {{1, 1}, {2, 5}}, {{{1, 1}}}, true},
        {true, {{1, 1}, {2, 3}}, {{{1, 2}, {2, 3}}}, false},
        {true, {{1, 1}, {2, 3}, {3, 6}}, {{{1, 1}, {2, 3}}, {{1, 1}, {2, 4}}}, true},
        {true, {{1, 1}, {2, 3}, {3, 6}}, {{{1, 1}, {2, 3}, {3, 7}}, {{1, 1}, {2, 4}, {3, 6}}}, false},
        {true, {{1, 1}, {2, 3}, {3, 6}}, {{{1, 1}, {2, 3}, {3, 7}}, {{1, 1}, {2, 4}, {3, 6}}, {{1, 1}, {2, 3}, {3, 6}}}, true},
        {false, {}, {{{1, 1}}}, true},
        {true, {{1, 1}}, {}, true},
    };
    u32 k = 0;
    for (const TRow& r : trows) {
        VolProblem vp;
        vp.N = 1;
        vp.node_csi.resize(1);
        MCsiInfo c;
        c.plugin = 1;
        c.has_topology = r.has_top;
        c.segments = r.top;
        vp.node_csi[0].push_back(c);
        MVolume m;
        m.driver = 1;
        m.accessible = r.accessible;
        vp.vol.push_back(m);
        if (vp.in_topology(0, 0) != r.expected) { fprintf(stderr, "selftest IsInTopology row %u: model %d, known answer %d\n", k, (int)!r.expected, (int)r.expected); ok = false; }
        ++k;
    }
    fprintf(stderr, "selftest: %zu checkVolume rows, %zu topology rows -> %s\n", sizeof rows / sizeof rows[0], sizeof trows / sizeof trows[0], ok ? "OK" : "FAIL");
    return ok ? 0 : 1;
}

// ---- functions ----
static int functions(u32 seed, u32 N) {
    VolProblem vp = make_volumes(seed, N, 12, 40);
    VolTables tb = vol_tables(vp);
    VolView view = tb.view();
    VolUsage use = vp.use0;
    const u32 S = (u32)vp.set.size();
    u64 task = 1;
    u64 checked = 0;
    auto check_choose = [&](u32 s, u32 n) -> bool {   // k_vol_choose's eleven words
        u32 want[VOL_MAX_MOUNTS], wfailed = 0;
        const u32 wn = vp.choose(use, s, n, task++, want, &wfailed);
        const u32 wfilter = vp.filter(use, s, n) ? 1u : 0u;
        std::vector<u32> out(VOL_MAX_MOUNTS + 3, 0xABABABABu);
        VolChooseArgs ca{view, s, n, out.data()};
        emu::launch(64, 0, [ca]() { k_vol_choose(ca); });
        bool ok = true;
        for (u32 q = 0; q < VOL_MAX_MOUNTS; ++q) ok = ok && out[q] == want[q];
        ok = ok && out[VOL_MAX_MOUNTS] == wn && out[VOL_MAX_MOUNTS + 1] == (wn ? 0u : wfailed) && out[VOL_MAX_MOUNTS + 2] == wfilter;
        if (!ok) {
            fprintf(stderr, "MISMATCH k_vol_choose set %u node %u:\n  emu  ", s, n);
            for (u32 q = 0; q < VOL_MAX_MOUNTS + 3; ++q) fprintf(stderr, " %d", (int)out[q]);
            fprintf(stderr, "\n  model");
            for (u32 q = 0; q < VOL_MAX_MOUNTS; ++q) fprintf(stderr, " %d", (int)want[q]);
            fprintf(stderr, " %u %u %u\n", wn, wn ? 0u : wfailed, wfilter);
        }
        ++checked;
        return ok;
    };
    auto check_word = [&](u32 s, u32 w) -> bool {   // the model's per-node filter, bit for bit; a bit beyond n_nodes is no node: 0
        u64 want = 0;
        for (u32 i = 0; i < 64; ++i)
            if (w * 64 + i < N && vp.filter(use, s, w * 64 + i)) want |= 1ull << i;
        const u64 got = vol_filter_word(view, s, w);
        if (got != want) fprintf(stderr, "MISMATCH vol_filter_word set %u word %u: emu %016llx model %016llx\n", s, w, got, want);
        return got == want;
    };
    for (u32 s = 1; s < S; ++s) {
        for (u32 n = 0; n < N; ++n)
            if (!check_choose(s, n)) return 1;
        for (u32 w = 0; w < tb.Wn; ++w)
            if (!check_word(s, w)) return 1;
    }
    // a sequence of placements: choose + reserve on both sides, the derived numbers after each one
    std::mt19937_64 g(seed * 77 + 5);
    u32 placed = 0, failed_choice = 0;
    for (u32 step = 0; step < 400; ++step) {
        const u32 s = 1 + (u32)(g() % (S - 1));
        u32 n = (u32)(g() % N);
        if (g() % 4 == 0) n = (g() % 2) ? 0 : N - 1;   // where the pinned volumes are
        if (!check_choose(s, n)) return 1;
        u32 want[VOL_MAX_MOUNTS], att[VOL_MAX_MOUNTS];
        const u64 id = task++;
        const u32 wn = vp.choose(use, s, n, id, want, nullptr);
        const u32 dn = vol_choose(view, s, n, att, nullptr);
        if (dn != wn) { fprintf(stderr, "MISMATCH vol_choose at step %u\n", step); return 1; }
        if (!wn) { ++failed_choice; continue; }
        vp.reserve(use, s, n, id, want, wn);
        vol_reserve(view, s, n, att, dn);
        ++placed;
        if (!same_dyn(vp, use, tb.vdyn, "after placement", step)) return 1;
        for (u32 z = 1; z < S; ++z)
            if (!check_word(z, 0) || !check_word(z, tb.Wn - 1) || !check_word(z, n >> 6)) return 1;
    }
    for (u32 s = 1; s < S; ++s)   // ... and every pair once more, against the usage the placements left
        for (u32 n = 0; n < N; n += 3)
            if (!check_choose(s, n)) return 1;
    print_reach("functions", vp.reach);
    fprintf(stderr, "functions seed %u N %u: %u volumes, %u sets, %llu (set, node) pairs, %u placements reserved, %u failed -> OK\n", seed, N, (u32)vp.vol.size(), S - 1, (unsigned long long)checked,
            placed, failed_choice);
    return 0;
}

// ---- topology ----
static int topology(u32 seed, u32 N) {
    VolProblem vp = make_volumes(seed, N, 12, 0);
    const u32 V = (u32)vp.vol.size(), Wn = (N + 63) / 64;
    std::vector<u32> node_csi_off, csi, csi_seg, vol_driver, vol_topo_off, topo_off, vol_seg;
    for (u32 n = 0; n < N; ++n) {
        node_csi_off.push_back((u32)csi.size() / 4);
        for (const MCsiInfo& c : vp.node_csi[n]) {
            csi.insert(csi.end(), {c.plugin, c.has_topology ? 1u : 0u, (u32)csi_seg.size() / 2, (u32)c.segments.size()});
            for (const auto& s : c.segments) csi_seg.insert(csi_seg.end(), {s.first, s.second});
        }
    }
    node_csi_off.push_back((u32)csi.size() / 4);
    for (u32 v = 0; v < V; ++v) {
        vol_driver.push_back(vp.vol[v].driver);
        vol_topo_off.push_back((u32)topo_off.size());
        for (const auto& t : vp.vol[v].accessible) {
            topo_off.push_back((u32)vol_seg.size() / 2);
            for (const auto& s : t) vol_seg.insert(vol_seg.end(), {s.first, s.second});
        }
    }
    vol_topo_off.push_back((u32)topo_off.size());
    topo_off.push_back((u32)vol_seg.size() / 2);
    csi.resize(csi.size() + 4, 0);
    csi_seg.resize(csi_seg.size() + 2, 0);
    vol_seg.resize(vol_seg.size() + 2, 0);
    std::vector<u64> T((size_t)V * Wn, 0xDDDDDDDDDDDDDDDDull);
    VolTopoArgs a{};
    a.n_nodes = N;
    a.n_words = Wn;
    a.n_vol = V;
    a.node_csi_off = node_csi_off.data();
    a.csi = csi.data();
    a.csi_seg = csi_seg.data();
    a.vol_driver = vol_driver.data();
    a.vol_topo_off = vol_topo_off.data();
    a.topo_off = topo_off.data();
    a.vol_seg = vol_seg.data();
    a.T = T.data();
    const u32 half = V / 2;   // two launches, as for more volumes than a grid's second dimension holds
    a.vol0 = 0;
    grid2((Wn * 64 + 255) / 256, half, 256, [a]() { k_vol_topology(a); });
    a.vol0 = half;
    grid2((Wn * 64 + 255) / 256, V - half, 256, [a]() { k_vol_topology(a); });
    // what the model's run came across
    u64 no_csi = 0, no_top = 0, twice = 0, no_acc = 0, zero_vs_missing = 0, fits = 0, misses = 0;
    for (u32 v = 0; v < V; ++v)
        for (u32 n = 0; n < N; ++n) {
            const MCsiInfo* top = nullptr;
            u32 of_plugin = 0;
            for (const MCsiInfo& c : vp.node_csi[n])
                if (c.plugin == vp.vol[v].driver) { if (!top) top = &c; ++of_plugin; }
            if (!top) ++no_csi;
            else if (!top->has_topology) ++no_top;
            if (of_plugin > 1) ++twice;
            if (vp.vol[v].accessible.empty()) ++no_acc;
            if (top && top->has_topology)
                for (const auto& t : vp.vol[v].accessible)
                    for (const auto& want : t) {
                        bool present = false;
                        for (const auto& s : top->segments) present = present || s.first == want.first;
                        if (!present && want.second == 0) ++zero_vs_missing;
                    }
            const bool want = vp.in_topology(v, n);
            (want ? fits : misses)++;
        }
    bool ok = true;
    for (u32 v = 0; v < V && ok; ++v)
        for (u32 w = 0; w < Wn && ok; ++w) {
            u64 want = 0;
            for (u32 i = 0; i < 64; ++i)
                if (w * 64 + i < N && vp.in_topology(v, w * 64 + i)) want |= 1ull << i;
            if (T[(size_t)v * Wn + w] != want) {
                fprintf(stderr, "MISMATCH T[volume %u][word %u]: emu %016llx model %016llx\n", v, w, T[(size_t)v * Wn + w], want);
                ok = false;
            }
        }
    fprintf(stderr, "reach topology: no_csi=%llu no_topology=%llu plugin_twice=%llu no_accessible=%llu zero_vs_missing=%llu fits=%llu misses=%llu\n", (unsigned long long)no_csi,
            (unsigned long long)no_top, (unsigned long long)twice, (unsigned long long)no_acc, (unsigned long long)zero_vs_missing, (unsigned long long)fits, (unsigned long long)misses);
    fprintf(stderr, "topology seed %u N %u: %u volumes in launches of %u and %u -> %s\n", seed, N, V, half, V - half, ok ? "OK" : "FAIL");
    return ok ? 0 : 1;
}

// ---- fitpairs ----
static int fitpairs(u32 seed, u32 n_seg, u32 hot, bool no_vol, bool plain) {
    const u32 N = n_seg + n_seg / 3 + 70, Wn = (N + 63) / 64;
    VolProblem vp = make_volumes(seed, N, 12, 30);
    VolTables tb = vol_tables(vp);
    const u32 n_sets = (u32)vp.set.size();
    std::mt19937_64 g(seed * 1000003ull + 17);
    auto rnd = [&](u32 k) { return (u32)(g() % k); };
    // nodes
    const u32 NC = 4, P = 4, K = 3, S = 9, gstride = N + 3;
    std::vector<u64> ready(Wn, 0), con((size_t)NC * Wn, 0), plat((size_t)NC * Wn, 0), plug((size_t)NC * Wn, 0);
    std::vector<i64> cpu(N), mem(N);
    std::vector<u32> total(N);
    std::vector<int32_t> gcnt((size_t)(K + 1) * gstride, 0);
    for (u32 n = 0; n < N; ++n) {
        if (rnd(12)) ready[n >> 6] |= 1ull << (n & 63);
        for (u32 c = 1; c < NC; ++c) {
            if (rnd(8)) con[(size_t)c * Wn + (n >> 6)] |= 1ull << (n & 63);
            if (rnd(8)) plat[(size_t)c * Wn + (n >> 6)] |= 1ull << (n & 63);
            if (rnd(8)) plug[(size_t)c * Wn + (n >> 6)] |= 1ull << (n & 63);
        }
        cpu[n] = (i64)rnd(10) * 1'000'000'000;
        mem[n] = (i64)rnd(10) << 30;
        total[n] = rnd(5);
        for (u32 k = 1; k <= K; ++k) gcnt[(size_t)k * gstride + n] = (int32_t)rnd(6);
    }
    // templates
    const u32 NT = 40;
    std::vector<FitTmpl> tm(NT);
    std::vector<u32> gkind, tm_svc(NT);
    std::vector<int32_t> gval;
    std::vector<std::vector<u32>> tm_ports(NT);
    for (u32 t = 0; t < NT; ++t) {
        FitTmpl& f = tm[t];
        memset(&f, 0, sizeof f);
        tm_svc[t] = t % S;   // (templates t and t + S: one service)
        if (rnd(3)) {
            f.rt.flags |= RT_RES;
            f.rt.cpu = (i64)rnd(3) * 500'000'000;
            f.rt.mem = (i64)rnd(3) << 29;
        }
        f.gen_off = (u32)gkind.size();
        if (rnd(3) == 0) {   // generic reservations enable the filter by themselves (filter.go:61-74); the same kind twice: the second Claim clamps at 0
            f.rt.flags |= RT_RES;
            const u32 k1 = 1 + rnd(K);
            gkind.push_back(k1);
            gval.push_back((int32_t)(1 + rnd(3)));
            if (rnd(2)) { gkind.push_back(rnd(2) ? k1 : 1 + rnd(K)); gval.push_back((int32_t)(1 + rnd(3))); }
        }
        f.n_gen = (u32)gkind.size() - f.gen_off;
        if (rnd(5) == 0) f.rt.cls_plug = 1 + rnd(NC - 1);
        if (rnd(5) == 0) f.rt.cls_con = 1 + rnd(NC - 1);
        if (rnd(5) == 0) f.rt.cls_plat = 1 + rnd(NC - 1);
        if (rnd(4) == 0) {
            f.rt.flags |= RT_PORTS;
            tm_ports[t].push_back(rnd(P));
            if (rnd(2)) tm_ports[t].push_back((tm_ports[t][0] + 1 + rnd(P - 1)) % P);
            f.n_ports = (u32)tm_ports[t].size();
        }
        if (rnd(4) == 0) { f.rt.flags |= RT_MAXREP; f.rt.maxrep = 1 + rnd(3); }
        if (rnd(8) == 0) f.rt.flags |= RT_UNCOUNTED;
        if (rnd(2) && !plain) f.mset = 1 + rnd(n_sets - 1);   // (plain: the model's VolumesFilter and choose lines are inert)
    }
    gkind.push_back(0);
    gval.push_back(0);
    // segments: distinct nodes in random order; pairs in segment order, the caller's order a permutation
    std::vector<u32> perm(N);
    for (u32 n = 0; n < N; ++n) perm[n] = n;
    std::shuffle(perm.begin(), perm.end(), g);
    std::swap(perm[0], *std::find(perm.begin(), perm.end(), N - 1));   // the hot segment: the node a single-node volume is pinned to
    std::vector<u32> seg_node(perm.begin(), perm.begin() + n_seg), seg_off(1, 0);
    std::vector<FitPair> pairs;
    std::vector<u32> port_slot;
    for (u32 s = 0; s < n_seg; ++s) {
        const u32 k = s == 0 && hot ? hot : 1 + rnd(4);
        const u32 fav = rnd(NT);
        for (u32 i = 0; i < k; ++i) {
            const u32 t = rnd(3) ? rnd(NT) : fav;   // the same template again: MaxReplicas reached inside a segment, a port taken by the pair in front
            FitPair q{0, t, s * S + tm_svc[t], (u32)port_slot.size()};
            for (u32 port : tm_ports[t]) port_slot.push_back(s * P + port);
            pairs.push_back(q);
        }
        seg_off.push_back((u32)pairs.size());
    }
    port_slot.push_back(0);
    const u32 NP = (u32)pairs.size();
    {
        std::vector<u32> idx(NP);
        for (u32 i = 0; i < NP; ++i) idx[i] = i;
        std::shuffle(idx.begin(), idx.end(), g);
        for (u32 i = 0; i < NP; ++i) pairs[i].idx = idx[i];
    }
    std::vector<u32> port_taken((size_t)n_seg * P), svc_cnt((size_t)n_seg * S);
    for (u32& x : port_taken) x = rnd(8) == 0;
    for (u32& x : svc_cnt) x = rnd(3);

    // ---- the model: a sequential loop over the pairs in segment order --------------------------------------------------------
    std::vector<i64> m_cpu = cpu, m_mem = mem;
    std::vector<u32> m_total = total, m_port = port_taken, m_svc = svc_cnt, m_att((size_t)NP * VOL_MAX_MOUNTS, VOL_NONE);
    std::vector<int32_t> m_gcnt = gcnt, m_out(NP, -99);
    VolUsage use = vp.use0;   // taskFitNode chooses and reserves nothing: never changed
    u64 hist[10] = {}, clamped = 0, drained_seg = 0, uncounted = 0, shared_port = 0, maxrep_inside = 0, task = 1;
    for (u32 s = 0; s < n_seg; ++s) {
        const u32 n = seg_node[s];
        auto bit = [&](const std::vector<u64>& rows, u32 row) { return ((rows[(size_t)row * Wn + (n >> 6)] >> (n & 63)) & 1) != 0; };
        if (!bit(ready, 0)) ++drained_seg;
        u32 booked_here = 0;
        for (u32 p = seg_off[s]; p < seg_off[s + 1]; ++p) {
            const FitPair& q = pairs[p];
            const FitTmpl& t = tm[q.tmpl];
            const bool res = (t.rt.flags & RT_RES) != 0;
            int ff = -1;
            if (!bit(ready, 0)) ff = 0;                                                                   // ReadyFilter
            if (ff < 0 && res && (t.rt.cpu > m_cpu[n] || t.rt.mem > m_mem[n])) ff = 1;                   // ResourceFilter
            for (u32 k = 0; ff < 0 && res && k < t.n_gen; ++k)
                if (m_gcnt[(size_t)gkind[t.gen_off + k] * gstride + n] < gval[t.gen_off + k]) ff = 1;
            if (ff < 0 && t.rt.cls_plug && !bit(plug, t.rt.cls_plug)) ff = 2;                             // PluginFilter
            if (ff < 0 && t.rt.cls_con && !bit(con, t.rt.cls_con)) ff = 3;                                // ConstraintFilter
            if (ff < 0 && t.rt.cls_plat && !bit(plat, t.rt.cls_plat)) ff = 4;                             // PlatformFilter
            if (ff < 0 && (t.rt.flags & RT_PORTS))                                                        // HostPortFilter
                for (u32 port : tm_ports[q.tmpl])
                    if (m_port[(size_t)s * P + port]) { ff = 5; if (booked_here) ++shared_port; }
            if (ff < 0 && (t.rt.flags & RT_MAXREP) && m_svc[(size_t)s * S + tm_svc[q.tmpl]] >= t.rt.maxrep) { ff = 6; if (booked_here) ++maxrep_inside; }   // MaxReplicasFilter
            if (ff < 0 && t.mset && (no_vol || !vp.filter(use, t.mset, n))) ff = 7;                       // VolumesFilter
            u32* row = &m_att[(size_t)q.idx * VOL_MAX_MOUNTS];
            if (ff < 0 && t.mset && vp.choose(use, t.mset, n, task++, row, nullptr) == 0) ff = 8;         // the prefix stays in the row
            m_out[q.idx] = ff;
            hist[ff + 1]++;
            if (ff >= 0) continue;
            ++booked_here;
            m_cpu[n] -= t.rt.cpu;
            m_mem[n] -= t.rt.mem;
            for (u32 k = 0; k < t.n_gen; ++k) {
                int32_t& c = m_gcnt[(size_t)gkind[t.gen_off + k] * gstride + n];
                c -= gval[t.gen_off + k];
                if (c < 0) { c = 0; ++clamped; }
            }
            if (t.rt.flags & RT_UNCOUNTED) ++uncounted;
            else {
                m_total[n] += 1;
                m_svc[(size_t)s * S + tm_svc[q.tmpl]] += 1;
            }
            for (u32 port : tm_ports[q.tmpl]) m_port[(size_t)s * P + port] = 1;
        }
    }

    // ---- the kernel ----------------------------------------------------------------------------------------------------------
    std::vector<int32_t> out(NP, -99);
    std::vector<u32> att((size_t)NP * VOL_MAX_MOUNTS, 0xABABABABu);
    const std::vector<VolDyn> vdyn0 = tb.vdyn;
    FitVolArgs av{};
    av.f.n_seg = n_seg;
    av.f.n_words = Wn;
    av.f.gstride = gstride;
    av.f.seg_node = seg_node.data();
    av.f.seg_off = seg_off.data();
    av.f.pairs = pairs.data();
    av.f.tm = tm.data();
    av.f.gkind = gkind.data();
    av.f.gval = gval.data();
    av.f.port_slot = port_slot.data();
    av.f.port_taken = port_taken.data();
    av.f.svc_cnt = svc_cnt.data();
    av.f.ready = ready.data();
    av.f.con = con.data();
    av.f.plat = plat.data();
    av.f.plug = plug.data();
    av.f.cpu = cpu.data();
    av.f.mem = mem.data();
    av.f.total = total.data();
    av.f.gcnt = gcnt.data();
    av.f.out = out.data();
    if (!no_vol) av.vol = tb.view();   // (no volume exists: every pointer null)
    av.att = att.data();
    if (plain) {   // k_fit_pairs gets FitArgs alone; every attachment row must stay as the caller left it
        grid2((n_seg + 255) / 256, 1, 256, [av]() { k_fit_pairs(av.f); });
        m_att.assign(m_att.size(), 0xABABABABu);
    } else {
        grid2((n_seg + 255) / 256, 1, 256, [av]() { k_fit_pairs_vol(av); });
    }

    bool ok = same("out", out, m_out, NP) && same("att", att, m_att, att.size()) && same("cpu", cpu, m_cpu, N) && same("mem", mem, m_mem, N) && same("total", total, m_total, N) &&
              same("gcnt", gcnt, m_gcnt, gcnt.size()) && same("svc_cnt", svc_cnt, m_svc, svc_cnt.size()) && same("port_taken", port_taken, m_port, port_taken.size());
    if (ok && memcmp(vdyn0.data(), tb.vdyn.data(), vdyn0.size() * sizeof(VolDyn)) != 0) { fprintf(stderr, "MISMATCH vdyn: the pass changed the volumes' usage\n"); ok = false; }
    print_reach("fitpairs", vp.reach);
    fprintf(stderr, "reach fitpairs shapes: pairs=%u ff_pass=%llu", NP, (unsigned long long)hist[0]);
    for (u32 f = 0; f < 9; ++f) fprintf(stderr, " ff%u=%llu", f, (unsigned long long)hist[f + 1]);
    fprintf(stderr, " clamped=%llu drained_segments=%llu uncounted=%llu port_of_a_pair_in_front=%llu maxrep_inside=%llu\n", (unsigned long long)clamped, (unsigned long long)drained_seg,
            (unsigned long long)uncounted, (unsigned long long)shared_port, (unsigned long long)maxrep_inside);
    fprintf(stderr, "fitpairs seed %u segments %u (hot %u) nodes %u pairs %u volumes %s -> %s\n", seed, n_seg, hot, N, NP, plain ? "unused" : no_vol ? "none" : "yes", ok ? "OK" : "FAIL");
    return ok ? 0 : 1;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "selftest") return selftest();
    if (mode == "functions" && argc >= 4) return functions(atoi(argv[2]), atoi(argv[3]));
    if (mode == "topology" && argc >= 4) return topology(atoi(argv[2]), atoi(argv[3]));
    if (mode == "fitpairs" && argc >= 5) return fitpairs(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), argc > 5 && argv[5][0] == 'z', argc > 5 && argv[5][0] == 'p');
    fprintf(stderr, "usage: %s selftest | functions seed N | topology seed N | fitpairs seed n_seg hot [z|p]\n", argv[0]);
    return 2;
}
