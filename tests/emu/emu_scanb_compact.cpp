// emu_scanb_compact.cpp — runs the COMPACT BATCHED instance of the scan resolver (swarmkit_amd/csrc/swp_scan.hpp: the probe k_scan_mark +
// k_scan_union, k_scan_fill_c, k_scan_lists_c, k_scanb<.., true>) on CPU fibers: clusters of more nodes than one workgroup's LDS holds,
// of which only `Nc` are in any class row — the kernels work on those, the sequential model of emu_model.hpp on ALL nodes; every output
// and every mutated array must agree. The harness restates the launcher's rule (launch_scan_compact): a stretch without host ports or
// generic reservations whose rows over the union fit in LDS (scan_lds_bc) goes to k_scanb<scanb_nq(n_c), true>, any other to
// k_scan<.., .., true>, and it says which. With `m` the batch goes through the block resolver, the compact batched scan and the block
// resolver again in thirds (bitmaps rebuilt at the hand-overs); with `k<len>` the scan is cut into stretches [0, len), [len, 2 len + 1),
// ... of growing odd lengths, each behind a probe of its own. On every run the compact class rows (scanb_rows_c, the function the
// kernel's prologue calls) are compared with the gather of the original rows through the map.
// TEST INFRASTRUCTURE (tests/test_emu_scanb_compact.py); not product.
//
//   emu_scanb_compact <seed> <N> <T> <S> <block> <order: 0 rr | 1 major | 2 random> <features 0..1> <Nc> [v] [m] [n: no descriptor ids] [k<len>]
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

// the class rows as the kernel's prologue builds them in LDS, copied out (one workgroup of SCANB_THREADS)
static void rows_out(ScanArgs s, u64* out) {
    u64* rows = reinterpret_cast<u64*>(wv::lds());
    scanb_rows_c(s, rows);
    wv::barrier();
    const u32 n = s.n_sc * ((s.n_c + 63u) / 64u);
    for (u32 x = wv::tid(); x < n; x += SCANB_THREADS) out[x] = rows[x];
}

int main(int argc, char** argv) {
    if (argc < 9) { fprintf(stderr, "usage: %s seed N T S block order features(0..1) Nc [v] [m] [n] [k<len>]\n", argv[0]); return 2; }
    const u32 seed = atoi(argv[1]), N = atoi(argv[2]), T = atoi(argv[3]), S = atoi(argv[4]), B = atoi(argv[5]);
    const int order = atoi(argv[6]), feat = atoi(argv[7]);
    const u32 Nc = atoi(argv[8]);
    bool verbose = false, mixed = false, no_tmpl = false;
    u32 cut = 0;
    for (int i = 9; i < argc; ++i) {
        if (argv[i][0] == 'v') verbose = true;
        if (argv[i][0] == 'm') mixed = true;
        if (argv[i][0] == 'n') no_tmpl = true;
        if (argv[i][0] == 'k') cut = (u32)atoi(argv[i] + 1);
    }
    if (N <= SCAN_MAXN || Nc < 1 || Nc > SCAN_MAXN || feat > 1 || S < 2) { fprintf(stderr, "more than %d nodes, of which 1 .. %d eligible; feature level 0 or 1; two services at least\n", SCAN_MAXN, SCAN_MAXN); return 2; }
    Problem p = make_problem(seed, N, T, S, order, feat);
    // The eligible nodes: exactly Nc, scattered — the last node first, then the first and the last bit of words, then random ones. They
    // are all valid; class row 0 is exactly this set, every other row what it was inside it. Service 0 asks for row 0, so a stretch
    // with a task of it has all Nc nodes in its union; the last service asks for row 9, one of the four empty ones (zones nobody is
    // in): its tasks find no node. From three services on service 1's tasks are not counted (RT_UNCOUNTED), from four on service 2 has
    // a replica limit of 2 a node.
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
    for (RTask& r : p.rt) {
        if (r.svc == 0) r.sc = 0;
        if (r.svc == S - 1) r.sc = 9;
        if (S >= 3 && r.svc == 1) r.flags |= RT_UNCOUNTED;
        if (S >= 4 && r.svc == 2) { r.flags |= RT_MAXREP; r.maxrep = 2; }
    }
    u32 empty_rows = 0;
    for (u32 c = 0; c < p.n_sc; ++c) {
        u64 any = 0;
        for (u32 w = 0; w < p.Wn; ++w) any |= p.sc[(size_t)c * p.Wn + w];
        empty_rows += any == 0;
    }
    if (empty_rows < 2) { fprintf(stderr, "fewer than two empty class rows\n"); return 2; }
    u32 outside = 0;   // pre-existing list entries on nodes outside the eligible set
    for (u32 e = 0; e < p.list_node.size(); ++e)
        if (p.list_node[e] != LIST_EMPTY && !((E[p.list_node[e] >> 6] >> (p.list_node[e] & 63)) & 1)) ++outside;
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
    // identical tasks: the first task with the same record (but for its list slot) — what the engine's batch preparation derives from the
    // descriptors (k_scanb: a task whose twin found no node earlier in the stretch is not looked at)
    std::vector<u32> tmpl(T);
    {
        std::map<std::tuple<u32, u32, u32, i64, i64, u32, u64>, u32> first;
        for (u32 j = 0; j < T; ++j) {
            const RTask& r = p.rt[j];
            tmpl[j] = first.emplace(std::make_tuple(r.svc, r.sc, r.flags, r.cpu, r.mem, r.pset, r.maxrep), j).first->second;
        }
    }
    a.tmpl = no_tmpl ? nullptr : tmpl.data();

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
    u32 probe_nc = 0, batched_launches = 0, plain_launches = 0, stretches = 0, shortest = 0xFFFFFFFFu, nq_seen = 0;
    size_t footprint = 0;
    bool probe_ok = true, rows_ok = true;
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
        ++stretches;
        shortest = std::min(shortest, j1 - j0);
        // ---- the probe: the class rows the stretch names, their union, its prefix sums and the map
        std::fill(used.begin(), used.end(), 0u);   // (the driver's memset)
        grid(64, 256, 0, [s]() { k_scan_mark(s); });
        grid(1, SCAN_THREADS, scan_union_lds(), [s]() { k_scan_union(s); });
        const u32 nc = cnc[0];
        probe_nc = std::max(probe_nc, nc);
        {
            std::vector<u64> want(p.Wn, 0);
            for (u32 j = j0; j < j1; ++j)
                for (u32 w = 0; w < p.Wn; ++w) want[w] |= p.sc[(size_t)p.rt[j].sc * p.Wn + w];
            u32 cnt = 0;
            for (u32 w = 0; w < p.Wn; ++w) {
                if (cu[w] != want[w]) { fprintf(stderr, "probe: union word %u differs\n", w); probe_ok = false; }
                cnt += (u32)__builtin_popcountll(want[w]);
            }
            if (nc != cnt) { fprintf(stderr, "probe: %u nodes counted, the union has %u\n", nc, cnt); probe_ok = false; }
            if (nc > SCAN_MAXN) { fprintf(stderr, "probe: the union has %u nodes\n", nc); return false; }
            for (u32 c = 0; c < nc && probe_ok; ++c) {
                const u32 n = cmap[c];
                if (n >= N || !((cu[n >> 6] >> (n & 63)) & 1) || (c && cmap[c - 1] >= n)) { fprintf(stderr, "probe: map[%u] = %u is not ascending inside the union\n", c, n); probe_ok = false; }
            }
            if (cmap[SCAN_MAXN] != 0xEEEEEEEEu) { fprintf(stderr, "probe: a write past the map's end\n"); probe_ok = false; }
        }
        if (!probe_ok) return false;
        if (nc == 0) {   // (nobody of the stretch can be placed anywhere: the driver's fits() refuses it, the rounds decide it)
            fprintf(stderr, "the stretch [%u, %u) has an empty union: not a case of this harness\n", j0, j1);
            return false;
        }
        s.n_c = nc;
        hmat.assign((size_t)S * nc, 0xABABABABu);
        emat.assign((size_t)S * nc, 0xCDCDCDCDu);
        s.hmat = hmat.data();
        s.emat = emat.data();
        grid(1024, 256, 0, [s]() { k_scan_fill_c(s); });
        for (u32 sv = 0; sv < S; ++sv) {
            emu::blockidx_y() = sv;
            grid(64, 256, 0, [s]() { k_scan_lists_c(s); });
        }
        emu::blockidx_y() = 0;
        {   // the compact class rows: bit c of row r is bit map[c] of the original row r; nothing beyond the union's last node
            const u32 Wc = (nc + 63) / 64;
            std::vector<u64> got((size_t)p.n_sc * Wc + 1, 0xEEEEEEEEEEEEEEEEull);
            u64* out = got.data();
            grid(1, SCANB_THREADS, (size_t)p.n_sc * Wc * 8, [s, out]() { rows_out(s, out); });
            for (u32 r = 0; r < p.n_sc; ++r)
                for (u32 w = 0; w < Wc; ++w) {
                    u64 want = 0;
                    for (u32 i = 0; i < 64 && w * 64 + i < nc; ++i) {
                        const u32 n = cmap[w * 64 + i];
                        want |= ((p.sc[(size_t)r * p.Wn + (n >> 6)] >> (n & 63)) & 1ull) << i;
                    }
                    if (got[(size_t)r * Wc + w] != want) { fprintf(stderr, "class rows: word %u of row %u is %llx, the gather through the map %llx\n", w, r, (unsigned long long)got[(size_t)r * Wc + w], (unsigned long long)want); rows_ok = false; }
                }
            if (got[(size_t)p.n_sc * Wc] != 0xEEEEEEEEEEEEEEEEull) { fprintf(stderr, "class rows: a write past the rows' end\n"); rows_ok = false; }
        }
        if (!rows_ok) return false;
        // the launcher's rule for the BATCHED instance: no generic reservations, no host ports in the stretch, every row over the union in LDS
        bool node_local = a.n_rg == 0;
        for (u32 j = j0; j < j1 && node_local; ++j)
            if (a.rt[j].flags & RT_PORTS) node_local = false;
        const size_t ldsb = scan_lds_bc(nc, s.n_svc, s.n_sc);
        footprint = std::max(footprint, ldsb);
        if (node_local && ldsb <= (size_t)160 * 1024 - 512) {
            nq_seen = std::max(nq_seen, scanb_nq(nc));
            switch (scanb_nq(nc)) {
                case 1: grid(1, SCANB_THREADS, ldsb, [s]() { k_scanb<1, true>(s); }); break;
                case 2: grid(1, SCANB_THREADS, ldsb, [s]() { k_scanb<2, true>(s); }); break;
                case 4: grid(1, SCANB_THREADS, ldsb, [s]() { k_scanb<4, true>(s); }); break;
                case 8: grid(1, SCANB_THREADS, ldsb, [s]() { k_scanb<8, true>(s); }); break;
                default: grid(1, SCANB_THREADS, ldsb, [s]() { k_scanb<16, true>(s); }); break;
            }
            ++rounds;
            ++batched_launches;
            if (blk.error) { fprintf(stderr, "k_scanb reported error %u\n", blk.error); return false; }
            return blk.pos == j1;
        }
        const bool lm = scan_lds_lm(nc, s.n_svc) <= (size_t)160 * 1024 - 512;   // the launcher's rule: the matrices in LDS when they fit
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
        ++plain_launches;
        if (blk.error) { fprintf(stderr, "k_scan reported error %u\n", blk.error); return false; }
        return blk.pos == j1;
    };
    auto scan_cut = [&](u32 j0, u32 j1) -> bool {   // stretches of cut, 2 cut + 1, 4 cut + 3, ... tasks: odd lengths, no multiple of the window
        if (!cut) return scan(j0, j1);
        u32 len = cut;
        for (u32 j = j0; j < j1;) {
            const u32 e = std::min(j1, j + len);
            if (!scan(j, e)) return false;
            j = e;
            len = 2 * len + 1;
        }
        return true;
    };
    bool ok = mixed ? (stretch(0, T / 3) && scan_cut(T / 3, 2 * T / 3) && stretch(2 * T / 3, T)) : scan_cut(0, T);
    if (!ok) return 3;

    ok = ok && same("out", em.out, ref.out, T) && same("cpu", em.cpu, ref.cpu, N) && same("mem", em.mem, ref.mem, N) && same("total", em.total, ref.total, N) &&
         same("X", em.X, ref.X, em.X.size()) && same("portmap", em.portmap, ref.portmap, em.portmap.size()) &&
         same("list_node", em.list_node, ref.list_node, em.list_node.size()) && same("list_svc", em.list_svc, ref.list_svc, em.list_svc.size()) &&
         same("list_fail", em.list_fail, ref.list_fail, em.list_fail.size());
    ok = ok && em.ctl.ncommit == ref.ctl.ncommit && em.ctl.ninf == ref.ctl.ninf;
    if (!ok) fprintf(stderr, "ncommit emu %u ref %u, ninf emu %u ref %u\n", em.ctl.ncommit, ref.ctl.ncommit, em.ctl.ninf, ref.ctl.ninf);
    ok = ok && same("log_node", em.log_node, ref.log_node, ref.ctl.ncommit) && same("log_task", em.log_task, ref.log_task, ref.ctl.ncommit) &&
         same("log_prev", em.log_prev, ref.log_prev, ref.ctl.ncommit) && same("last", em.last, ref.last, N) &&
         same("inf_task", em.inf_task, ref.inf_task, ref.ctl.ninf) && same("inf_pos", em.inf_pos, ref.inf_pos, ref.ctl.ninf);
    // the incrementally maintained bitmaps against a rebuild from the final node rows (same base: levels are relative to it)
    if (ok && mixed) {
        std::vector<u64> planes2 = planes, rr2 = rr;
        grid((p.Wn + 3) / 4, 256, 0, [a]() { k_r6_rows(a); });
        ok = same("planes", planes2, planes, planes.size()) && same("rr", rr2, rr, (size_t)(n_dc + n_dm) * p.Wn);
    }
    u32 n_maxrep = 0, n_unc = 0, n_heavy = 0;
    for (u32 j = 0; j < T; ++j) {
        n_maxrep += (p.rt[j].flags & RT_MAXREP) != 0;
        n_unc += (p.rt[j].flags & RT_UNCOUNTED) != 0;
        n_heavy += (p.rt[j].flags & RT_RES) && p.rt[j].cpu >= 40 * p.UC;
    }
    if (verbose || !ok) {
        fprintf(stderr, "class rows over the compact space equal the gather of the original rows through the map (%u stretches): %s\n", stretches, rows_ok && probe_ok ? "OK" : "FAIL");
        fprintf(stderr, "footprint: scan_lds_bc(%u, %u, %u) = %zu bytes of %zu -> %s\n", probe_nc, S, p.n_sc, footprint, (size_t)160 * 1024 - 512,
                footprint <= (size_t)160 * 1024 - 512 ? "fits" : "does not fit: the one-task-a-barrier compact instance (k_scan) runs");
    }
    fprintf(stderr, "seed %u N %u T %u S %u block %u order %d feat %d: union %u nq %u | placed %u inf %u skipped %u | k_scanb launches %u k_scan launches %u shortest stretch %u | tasks with maxrep %u uncounted %u heavy %u, list entries outside the union %u | rounds %llu -> %s\n",
            seed, N, T, S, B, order, feat, probe_nc, nq_seen, em.ctl.ncommit, em.ctl.ninf, blk.scan_skipped, batched_launches, plain_launches, shortest, n_maxrep, n_unc, n_heavy, outside,
            (unsigned long long)rounds, ok ? "OK" : "FAIL");
    return ok ? 0 : 1;
}
