// emu_scan_compact.cpp — runs the COMPACT instance of the scan resolver (swarmkit_amd/csrc/swp_scan.hpp: k_scan_mark, k_scan_union,
// k_scan_fill_c, k_scan_lists_c, k_scan<.., .., true>) on CPU fibers: clusters of more nodes than one workgroup's LDS holds, of which
// only `Nc` are in any class row — the kernels work on those, the sequential model of emu_model.hpp on ALL nodes; every output and every
// mutated array must agree. With `m` the batch goes through the block resolver, the compact scan and the block resolver again in thirds
// (bitmaps rebuilt at the hand-overs). The probe's arithmetic is checked on every run: the map is ascending, its inverse agrees with it,
// the matrices hold exactly the list entries of nodes inside the union. TEST INFRASTRUCTURE (tests/test_emu_scan_compact.py); not product.
//
//   emu_scan_compact <seed> <N> <T> <S> <block> <order: 0 rr | 1 major | 2 random> <features 0..3> <Nc> [v] [m] [g: matrices in global memory]
#include "wv_emu.hpp"

#define SWP_R6_KERNELS
#include "../../swarmkit_amd/csrc/swp_resolve6.hpp"
#define SWP_SCAN_KERNELS
#include "../../swarmkit_amd/csrc/swp_scan.hpp"

#include "emu_model.hpp"

template <class F>
static void grid(u32 blocks, u32 threads, size_t lds, F body) {
    for (u32 b = 0; b < blocks; ++b) {
        emu::blockidx() = b;
        emu::launch(threads, lds, body);
    }
    emu::blockidx() = 0;
}

int main(int argc, char** argv) {
    if (argc < 9) { fprintf(stderr, "usage: %s seed N T S block order features(0..3) Nc [v] [m] [g]\n", argv[0]); return 2; }
    const u32 seed = atoi(argv[1]), N = atoi(argv[2]), T = atoi(argv[3]), S = atoi(argv[4]), B = atoi(argv[5]);
    const int order = atoi(argv[6]), feat = atoi(argv[7]);
    const u32 Nc = atoi(argv[8]);
    bool verbose = false, mixed = false, no_lm = false;
    for (int i = 9; i < argc; ++i) {
        if (argv[i][0] == 'v') verbose = true;
        if (argv[i][0] == 'm') mixed = true;
        if (argv[i][0] == 'g') no_lm = true;
    }
    if (N <= SCAN_MAXN || Nc < 1 || Nc > SCAN_MAXN) { fprintf(stderr, "more than %d nodes, of which 1 .. %d eligible\n", SCAN_MAXN, SCAN_MAXN); return 2; }
    Problem p = make_problem(seed, N, T, S, order, feat);
    // The eligible nodes: exactly Nc, scattered — the last node first, then the first and the last bit of words, then random ones. They
    // are all valid; class row 0 is exactly this set, every other row what it was inside it (two rows in eleven are empty: tasks that
    // find no node). Service 0 asks for row 0, so a stretch with a task of it has all Nc nodes in its union.
    std::vector<u64> E(p.Wn, 0);
    {
        std::mt19937_64 g(0xC0FFEEull * (seed + 1));
        u32 have = 0;
        auto take = [&](u32 n) {
            if (have == Nc || n >= N || ((E[n >> 6] >> (n & 63)) & 1)) return;
            E[n >> 6] |= 1ull << (n & 63);
            ++have;
        };
        take(N - 1);
        const u32 edge[] = {63, 64, 127, 4095, 4096, (p.Wn - 1) * 64, (p.Wn - 1) * 64 - 1, 0};
        for (u32 n : edge) take(n);
        while (have < Nc) take((u32)(g() % N));
    }
    for (u32 w = 0; w < p.Wn; ++w) p.valid[w] |= E[w];
    for (u32 c = 0; c < p.n_sc; ++c)
        for (u32 w = 0; w < p.Wn; ++w) p.sc[(size_t)c * p.Wn + w] = c == 0 ? E[w] : p.sc[(size_t)c * p.Wn + w] & E[w];
    for (RTask& r : p.rt)
        if (r.svc == 0) r.sc = 0;
    // demand classes over the raw reservations (what the engine's batch preparation does)
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
    std::vector<u64> F;
    scan_window(p, ref, 0, T, F);
    ref_window(p, ref, 0, T, F);   // the model: every task over ALL N nodes

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
    a.task_rows = 0u;
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
    auto build = [&]() {
        grid(1, 1024, 256, [a]() { k_r6_minmax(a); });
        grid((p.Wn + 3) / 4, 256, 0, [a]() { k_r6_rows(a); });
    };
    auto stretch = [&](u32 j0, u32 j1) -> bool {
        build();
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
    // the probe's buffers: poisoned, the map one cell longer than the kernel may write
    std::vector<u32> used(p.n_sc, 0xEEEEEEEEu), cpre(p.Wn, 0xEEEEEEEEu), cmap(SCAN_MAXN + 1, 0xEEEEEEEEu), cnc(1, 0xEEEEEEEEu);
    std::vector<u64> cu(p.Wn, 0xEEEEEEEEEEEEEEEEull);
    std::vector<u32> hmat, emat;
    u32 probe_nc = 0;
    bool probe_ok = true;
    auto scan = [&](u32 j0, u32 j1) -> bool {
        ScanArgs s{};
        s.a = a;
        s.j0 = j0;
        s.j1 = j1;
        s.n_svc = S;
        s.n_sc = p.n_sc;
        s.cused = used.data();
        s.cu = cu.data();
        s.cpre = cpre.data();
        s.cmap = cmap.data();
        s.cnc = cnc.data();
        blk.error = 0;
        // ---- the probe: the class rows the stretch names, their union, its prefix sums and the map
        std::fill(used.begin(), used.end(), 0u);   // (the driver's memset)
        grid(64, 256, 0, [s]() { k_scan_mark(s); });
        grid(1, SCAN_THREADS, scan_union_lds(), [s]() { k_scan_union(s); });
        const u32 nc = cnc[0];
        probe_nc = nc;
        {
            std::vector<u64> want(p.Wn, 0);
            for (u32 j = j0; j < j1; ++j)
                for (u32 w = 0; w < p.Wn; ++w) want[w] |= p.sc[(size_t)p.rt[j].sc * p.Wn + w];
            u32 cnt = 0;
            for (u32 w = 0; w < p.Wn; ++w) {
                if (cu[w] != want[w]) { fprintf(stderr, "probe: union word %u differs\n", w); probe_ok = false; }
                if (cpre[w] != cnt) { fprintf(stderr, "probe: prefix of word %u is %u, want %u\n", w, cpre[w], cnt); probe_ok = false; }
                cnt += (u32)__builtin_popcountll(want[w]);
            }
            if (nc != cnt) { fprintf(stderr, "probe: %u nodes counted, the union has %u\n", nc, cnt); probe_ok = false; }
            if (nc > SCAN_MAXN) { fprintf(stderr, "probe: the union has %u nodes\n", nc); return false; }
            for (u32 c = 0; c < nc && probe_ok; ++c) {
                const u32 n = cmap[c];
                if (n >= N || !((cu[n >> 6] >> (n & 63)) & 1) || (c && cmap[c - 1] >= n)) { fprintf(stderr, "probe: map[%u] = %u is not ascending inside the union\n", c, n); probe_ok = false; }
                else if (scan_c_of(cu.data(), cpre.data(), n) != c) { fprintf(stderr, "probe: the inverse of map[%u] = %u is %u\n", c, n, scan_c_of(cu.data(), cpre.data(), n)); probe_ok = false; }
            }
            if (cmap[SCAN_MAXN] != 0xEEEEEEEEu) { fprintf(stderr, "probe: a write past the map's end\n"); probe_ok = false; }
        }
        if (!probe_ok) return false;
        if (nc == 0) { fprintf(stderr, "the stretch has an empty union: not a case of this harness\n"); return false; }
        s.n_c = nc;
        hmat.assign((size_t)S * nc, 0xABABABABu);
        emat.assign((size_t)S * nc, 0xCDCDCDCDu);
        s.hmat = hmat.data();
        s.emat = emat.data();
        const std::vector<u32> ln0 = em.list_node, ls0 = em.list_svc, lf0 = em.list_fail;
        grid(1024, 256, 0, [s]() { k_scan_fill_c(s); });
        for (u32 sv = 0; sv < S; ++sv) {
            emu::blockidx_y() = sv;
            grid(64, 256, 0, [s]() { k_scan_lists_c(s); });
        }
        emu::blockidx_y() = 0;
        {   // the matrices: a cell per list entry inside the union and no other; the lists themselves as they were
            size_t cells = 0, inside = 0;
            for (u32 sv = 0; sv < S; ++sv)
                for (u32 e = p.list_off[sv]; e < p.list_off[sv + 1]; ++e) {
                    const u32 n = em.list_node[e];
                    if (n == LIST_EMPTY || !((cu[n >> 6] >> (n & 63)) & 1)) continue;
                    ++inside;
                    if (emat[(size_t)sv * nc + scan_c_of(cu.data(), cpre.data(), n)] != e) { fprintf(stderr, "probe: entry %u of service %u (node %u) is not in its cell\n", e, sv, n); probe_ok = false; }
                }
            for (u32 x : emat) cells += x != LIST_EMPTY;
            if (cells != inside) { fprintf(stderr, "probe: %zu cells for %zu entries inside the union\n", cells, inside); probe_ok = false; }
            if (em.list_node != ln0 || em.list_svc != ls0 || em.list_fail != lf0) { fprintf(stderr, "probe: k_scan_lists_c changed a list\n"); probe_ok = false; }
        }
        if (!probe_ok) return false;
        const bool lm = scan_lds_lm(nc, s.n_svc) <= (size_t)160 * 1024 - 512 && !no_lm;   // the launcher's rule: the matrices in LDS when they fit
        const size_t lds = lm ? scan_lds_lm(nc, s.n_svc) : scan_lds(nc);
        switch (scan_nq(nc) * 2 + (lm ? 1 : 0)) {   // the instance the launcher picks for this union
            case 2: grid(1, SCAN_THREADS, lds, [s]() { k_scan<1, false, true>(s); }); break;
            case 3: grid(1, SCAN_THREADS, lds, [s]() { k_scan<1, true, true>(s); }); break;
            case 4: grid(1, SCAN_THREADS, lds, [s]() { k_scan<2, false, true>(s); }); break;
            case 5: grid(1, SCAN_THREADS, lds, [s]() { k_scan<2, true, true>(s); }); break;
            case 8: grid(1, SCAN_THREADS, lds, [s]() { k_scan<4, false, true>(s); }); break;
            default: grid(1, SCAN_THREADS, lds, [s]() { k_scan<4, true, true>(s); }); break;
        }
        ++rounds;
        if (blk.error) { fprintf(stderr, "k_scan reported error %u\n", blk.error); return false; }
        return blk.pos == j1;
    };
    bool ok = mixed ? (stretch(0, T / 3) && scan(T / 3, 2 * T / 3) && stretch(2 * T / 3, T)) : scan(0, T);
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
    // the incrementally maintained bitmaps against a rebuild from the final node rows (same base: levels are relative to it)
    if (ok && mixed) {
        std::vector<u64> planes2 = planes, rr2 = rr, rg2 = rg;
        grid((p.Wn + 3) / 4, 256, 0, [a]() { k_r6_rows(a); });
        ok = same("planes", planes2, planes, planes.size()) && same("rr", rr2, rr, (size_t)(n_dc + n_dm) * p.Wn) && same("rg", rg2, rg, p.rg_kind.size() * p.Wn);
    }
    u32 n_ports = 0, n_gen = 0, n_maxrep = 0, n_unc = 0;
    for (u32 j = 0; j < T; ++j) {
        n_ports += (p.rt[j].flags & RT_PORTS) != 0;
        n_maxrep += (p.rt[j].flags & RT_MAXREP) != 0;
        n_unc += (p.rt[j].flags & RT_UNCOUNTED) != 0;
        n_gen += !p.tg.empty() && p.tg[j] != 0;
    }
    if (verbose || !ok)
        fprintf(stderr, "probe: union of %u nodes (asked for %u), map ascending, inverse and matrices agree: %s\n", probe_nc, Nc, probe_ok ? "OK" : "FAIL");
    fprintf(stderr, "seed %u N %u T %u S %u block %u order %d feat %d: union %u | placed %u inf %u | tasks with ports %u generic %u maxrep %u uncounted %u | rounds %llu -> %s\n", seed, N, T, S, B, order, feat,
            probe_nc, em.ctl.ncommit, em.ctl.ninf, n_ports, n_gen, n_maxrep, n_unc, (unsigned long long)rounds, ok ? "OK" : "FAIL");
    return ok ? 0 : 1;
}
