// emu_resolve6_heads.cpp — emu_resolve6_window.cpp's run of the block resolver's kernel source against the sequential model, counting what
// the hand-over of the task heads through LDS adds (swp_resolve6.hpp, r6_commit_t: the staging wave leaves a task's flags in its L_cur
// word and its descriptor id in its pick slot; wave 0 reads a group's set-up from LDS only). It REPORTS, on a "reach heads:" line next to
// the window driver's "reach window:" line, the paths a run came across in groups >= 2 — the groups a HELPER staged — so that
// tests/test_emu_resolve6_heads.py asserts them.
// TEST INFRASTRUCTURE; not product.
//
//   emu_resolve6_heads <seed> <N> <T> <S> <block> <order: 0 rr | 1 major | 2 random> <features 0..4> [v] [s] [t] [c|f] [n] [m<k>] [a]
//       [L<k>: windows of k entries through R6Args.win] [x: no extension] [W<k>: a window of k entries through R6Args.dbg]
//       [U<k>: exactly the tasks k - 1, 2k - 1, ... are uncounted (whatever their services say): a cut every k tasks]
//       [E: the batch's last service already runs on every valid node: its tasks have no plain candidate and take the best entry of its
//           exception list — in round-robin order a round is cut in front of one every S tasks, and the next round places it first]
//       [P: R6Args.dbg bit 4, the kernel's section timers — and with them Blk6.dbg_late_runs, the picks the runs-by-rank path took in groups >= 2]
//       [R: R6Args.no_runs = 1 (the engine sets it for a batch without a run of >= 8 identical tasks)]
#include "wv_emu.hpp"

#define SWP_R6_KERNELS
#include "../../swarmkit_amd/csrc/swp_resolve6.hpp"

#include <tuple>

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
    if (argc < 8) { fprintf(stderr, "usage: %s seed N T S block order features(0..4) [v] [s] [t] [c|f] [n] [m<k>] [a] [h] [w] [L<k>] [x] [W<k>] [U<k>] [E] [P] [R]\n", argv[0]); return 2; }
    const u32 seed = atoi(argv[1]), N = atoi(argv[2]), T = atoi(argv[3]), S = atoi(argv[4]), B = atoi(argv[5]);
    const int order = atoi(argv[6]), feat = atoi(argv[7]);
    bool verbose = false, split = false, task_rows = false, twins = true, compact = false, fused = false, adjacent = false, hot = false, writer = false;
    bool no_ext = false, no_runs = false, exc_last = false, timers = false;
    u32 every = 10, dbg_win = 0, arg_win = 0, unc_every = 0;
    for (int i = 8; i < argc; ++i) {
        if (argv[i][0] == 'v') verbose = true;
        if (argv[i][0] == 's') split = true;
        if (argv[i][0] == 't') task_rows = true;   // rows per task of the block, rebuilt every round, instead of demand-class rows
        if (argv[i][0] == 'c') compact = true;     // a compact index of the lowest level's nodes in front of every round (k_r6_compact)
        if (argv[i][0] == 'f') compact = fused = true;   // ... built at the END of k_r6_commit_c for the next round (R6Args.compact == 2); k_r6_compact itself only in front of every fifth round (a chunk's first)
        if (argv[i][0] == 'n') twins = false;      // lists start at the level's first candidate (R6Args.tmpl == nullptr: what the shard drivers run)
        if (argv[i][0] == 'm') every = std::max(atoi(argv[i] + 1), 1);
        if (argv[i][0] == 'a') adjacent = true;
        if (argv[i][0] == 'h') hot = true;
        if (argv[i][0] == 'w') writer = true;
        if (argv[i][0] == 'x') no_ext = true;
        if (argv[i][0] == 'R') no_runs = true;
        if (argv[i][0] == 'E') exc_last = true;
        if (argv[i][0] == 'P') timers = true;
        if (argv[i][0] == 'U') unc_every = (u32)std::max(atoi(argv[i] + 1), 1);
        if (argv[i][0] == 'L') arg_win = (u32)atoi(argv[i] + 1);   // R6Args.win: rows of the windows in LDS (the engine: 32 for batches of runs)
        if (argv[i][0] == 'W') dbg_win = (u32)atoi(argv[i] + 1) & 31u;
    }
    const bool mounts = feat >= 4;
    if (mounts && compact) { fprintf(stderr, "a batch with cluster mounts runs without the compact index (launch_r6_rounds)\n"); return 2; }
    Problem p = make_problem(seed, N, T, S, order, feat);
    if (exc_last) {   // entries for every valid node in front of the last service's list (nothing behind it moves but its own tasks' slots)
        const u32 e = S - 1, at = p.list_off[e];
        std::vector<u32> add;
        for (u32 n = 0; n < N; ++n)
            if (((p.valid[n >> 6] >> (n & 63)) & 1) && !((p.X[(size_t)e * p.Wn + (n >> 6)] >> (n & 63)) & 1)) add.push_back(n);
        p.list_node.insert(p.list_node.begin() + at, add.begin(), add.end());
        p.list_svc.insert(p.list_svc.begin() + at, add.size(), 1u);
        p.list_fail.insert(p.list_fail.begin() + at, add.size(), 0u);
        for (u32 n : add) p.X[(size_t)e * p.Wn + (n >> 6)] |= 1ull << (n & 63);
        p.list_off[S] += (u32)add.size();
        for (u32 j = 0; j < T; ++j)
            if (p.rt[j].svc == e) {
                p.rt[j].slot += (u32)add.size();
                p.rt[j].sc = 0;   // (the class of all valid nodes; no replica limit: every entry counts)
                p.rt[j].flags &= ~(u32)(RT_MAXREP | RT_PORTS | RT_UNCOUNTED);
            }
    }
    for (u32 j = 0; unc_every && j < T; ++j) p.rt[j].flags = (p.rt[j].flags & ~(u32)RT_UNCOUNTED) | (j % unc_every == unc_every - 1u ? (u32)RT_UNCOUNTED : 0u);
    VolProblem vp;
    MountRun mr;
    VolTables vt;
    if (mounts) {
        vp = make_volumes(seed, N, 8, 30, hot ? 6 : 0);
        mr = make_mounts(vp, seed, T, every, adjacent, hot ? 6 : 0, false, writer);
        vt = vol_tables(vp);
    }
    // demand classes over the raw reservations (what the engine's batch preparation does)
    std::set<i64> sc, sm;
    for (const RTask& r : p.rt)
        if (r.flags & RT_RES) { sc.insert(r.cpu); sm.insert(r.mem); }
    if (sc.size() > 255 || sm.size() > 255) { fprintf(stderr, "too many demand classes for this harness\n"); return 2; }
    std::vector<i64> thr;
    std::map<i64, u32> ic, im;
    for (i64 v : sc) { ic[v] = (u32)thr.size(); thr.push_back(v); }
    u32 n_dc = (u32)sc.size();
    for (i64 v : sm) { im[v] = (u32)thr.size() - n_dc; thr.push_back(v); }
    u32 n_dm = (u32)sm.size();
    for (RTask& r : p.rt)
        if (r.flags & RT_RES) r.flags |= (ic[r.cpu] << RT_DC_SHIFT) | (im[r.mem] << RT_DM_SHIFT);

    if (task_rows) n_dc = n_dm = 0;
    State ref = initial_state(p), em = initial_state(p);
    std::vector<u64> F;
    scan_window(p, ref, 0, T, F);
    ref_window(p, ref, 0, T, F, mounts ? &mr : nullptr);

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
    std::vector<R6PropExt> ext(B);
    a.ext = no_ext ? nullptr : ext.data();
    a.dbg = (dbg_win << 12) | (timers ? 16u : 0u);
    a.win = arg_win;
    a.no_runs = no_runs ? 1u : 0u;
    // what the run came across in groups >= 2 of a round (tasks 128 ... of its block): cuts in front of an exception-list task or a second
    // task with cluster mounts (why 2), behind an uncounted task (why 3), unplaceable tasks decided there
    // (a why-2 cut is told apart by the task it lies in front of: one with mounts, or one the next round places from its exception list)
    u64 late_cut_exception = 0, late_cut_mount = 0, late_cut_uncounted = 0, late_unplaceable = 0, late_exception_first = 0, late_run_groups = 0;
    // what the run came across
    u64 long_lists = 0, longest = 0, rounds_two_groups = 0, cuts_late = 0, window_cut_then_decided = 0;
    std::vector<u64> trows((size_t)B * p.Wn, 0x7777777777777777ull);
    a.task_rows = task_rows ? 1u : 0u;
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

    std::vector<u64> vrows(std::max<size_t>(mr.csi_set.size(), 1) * p.Wn, 0x9999999999999999ull);
    std::vector<u32> att(std::max<size_t>(mr.csi_set.size(), 1) * VOL_MAX_MOUNTS, VOL_NONE);
    if (mounts) {
        a.csi_of = mr.csi_of.data();
        a.csi_set = mr.csi_set.data();
        a.vrows = vrows.data();
        a.att = att.data();
        a.vol = vt.view();
    }
    u64 cut_at_mount = 0;   // rounds that ended early, in front of a task with mounts, having decided one

    // identical tasks: the first task with the same record (but for its list slot) and generic set — what the engine's batch preparation
    // derives from the descriptors
    std::vector<u32> tmpl(T);
    {
        std::map<std::tuple<u32, u32, u32, i64, i64, u32, u64, u32, u32>, u32> first;
        for (u32 j = 0; j < T; ++j) {
            const RTask& r = p.rt[j];
            tmpl[j] = first.emplace(std::make_tuple(r.svc, r.sc, r.flags, r.cpu, r.mem, r.pset, r.maxrep, p.tg.empty() ? 0u : p.tg[j], mounts && mr.is(j) ? mr.csi_set[mr.csi_of[j]] : 0u), j).first->second;
        }
    }
    a.tmpl = twins ? tmpl.data() : nullptr;
    std::vector<u64> cmask(p.Wn, 0xDDDDDDDDDDDDDDDDull);
    std::vector<u32> crank(p.Wn, 0xDDDDDDDDu), cidx(r6_compact_cap(p.Wn), 0xDDDDDDDDu);
    a.compact = compact ? (fused && !task_rows ? 2u : 1u) : 0u;
    a.cbase = p.valid.data();   // (the harness has no drained nodes: every valid node is ready)
    a.cmask = cmask.data();
    a.crank = crank.data();
    a.cidx = cidx.data();
    u64 crounds_checked = 0;

    u64 rounds = 0;
    u32 pending_cut = R6_NONE, pending_seen = R6_NONE;
    auto build = [&]() {
        grid(1, 1024, 256, [a]() { k_r6_minmax(a); });
        grid((p.Wn + 3) / 4, 256, 0, [a]() { k_r6_rows(a); });
    };
    // the instance launch_r6_rounds picks for the node set (without a compact index)
    auto propose_plain = [&]() {
        if (p.Wn <= R6_TINY_WORDS && B > 1024u) grid(B, 64 * R6_PW_TINY, r6_propose_lds(p.Wn), [a]() { k_r6_propose_tiny(a); });
        else if (p.Wn <= R6_SMALL_WORDS) grid(B, 64 * R6_PW, r6_propose_lds(p.Wn), [a]() { k_r6_propose_small(a); });
        else grid(B, 64 * R6_PW, r6_propose_lds(p.Wn), [a]() { k_r6_propose(a); });
    };
    auto stretch = [&](u32 j0, u32 j1) -> bool {
        build();
        if (blk.error) { fprintf(stderr, "build reported error %u\n", blk.error); return false; }
        blk.pos = j0;
        blk.end = j1;
        while (blk.pos < blk.end) {
            const u32 before = blk.pos;
            for (R6Prop& q : prop) memset(&q, 0xEE, sizeof q);
            for (R6PropExt& q : ext) memset(&q, 0xEE, sizeof q);
            const u32 wc_before = blk.cut_window, cnt_round = std::min(B, blk.end - blk.pos);
            const u32 ce_before = blk.cut_exception, cu_before = blk.cut_uncounted, ninf_before = em.ctl.ninf;
            if (task_rows)
                for (u32 gy = 0; gy < (B + 63) / 64; ++gy) {   // grid (words / 4, groups of the block)
                    emu::blockidx_y() = gy;
                    grid((p.Wn + 3) / 4, 256, (size_t)B * 16, [a]() { k_r6_taskrows(a); });
                }
            emu::blockidx_y() = 0;
            if (compact) {
                if (a.compact != 2u || rounds % 5 == 0 || blk.pos == j0) grid(1, 1024, 256, [a]() { k_r6_compact(a); });
                // the index against its definition: the ready nodes on ONE level, in node order, no more than a quarter of the node set;
                // whether that level is the first task's is checked by the outcome (a wrong level only makes the index useless)
                std::vector<u32> want;
                for (u32 n = 0; n < N && blk.clevel != R6_NONE; ++n)
                    if (((p.valid[n >> 6] >> (n & 63)) & 1) && em.total[n] == blk.base + blk.clevel) want.push_back(n);
                const u32 cnt = (u32)want.size();
                const bool on = cnt != 0 && cnt <= r6_compact_cap(p.Wn);
                if (blk.csize != (on ? cnt : 0u)) { fprintf(stderr, "compact index: size %u on level %u, expected %u\n", blk.csize, blk.clevel, on ? cnt : 0u); return false; }
                for (u32 i = 0; on && i < cnt; ++i)
                    if (cidx[i] != want[i]) { fprintf(stderr, "compact index: position %u is node %u, expected %u\n", i, cidx[i], want[i]); return false; }
                if (on) ++crounds_checked;
                grid(B, 64 * R6_PW, r6_propose_lds(p.Wn), [a]() { k_r6_propose_c(a); });
                grid(1, R6_COMMIT_THREADS, r6_commit_lds(p.Wn, B, n_dc + n_dm, true, arg_win), [a]() { k_r6_commit_c(a); });
            } else if (mounts) {
                for (u32 by = 0; by < B; ++by) {   // grid (words / 256, block)
                    emu::blockidx_y() = by;
                    grid((p.Wn + 255) / 256, 256, 0, [a]() { k_r6_volrows(a); });
                }
                emu::blockidx_y() = 0;
                propose_plain();
                grid(1, R6_COMMIT_THREADS, r6_commit_lds(p.Wn, B, n_dc + n_dm, false, arg_win), [a]() { k_r6_commit_v(a); });
                if (blk.pos < std::min(before + B, blk.end) && mr.is(blk.pos))
                    for (u32 j = before; j < blk.pos; ++j)
                        if (mr.is(j)) { ++cut_at_mount; break; }
            } else {
                propose_plain();
                grid(1, R6_COMMIT_THREADS, r6_commit_lds(p.Wn, B, n_dc + n_dm, false, arg_win), [a]() { k_r6_commit(a); });
            }
            for (u32 j = 0; j < cnt_round; ++j)   // (read behind the commit: the proposals of the round are still there)
                if (prop[j].level != R6_NONE) {
                    const u32 nc = prop[j].n_cand & 0x7FFFFFFFu;
                    if (nc > 2 * R6_CAND) ++long_lists;
                    longest = std::max<u64>(longest, nc);
                    if (nc > (no_ext ? 2u * R6_CAND : (u32)R6_LIST)) { fprintf(stderr, "a list of %u entries\n", nc); return false; }
                }
            {
                const u32 did = blk.pos - before;
                // a cut with why 2 lies in front of task `did` of the block, one with why 3 behind task `did - 1`
                if (blk.cut_exception != ce_before && did >= 128u && did < cnt_round) ++(mounts && mr.is(blk.pos) ? late_cut_mount : late_cut_exception);
                // groups >= 2 of the round whose first eight tasks are one run of identical tasks, all placed in this round: where the
                // matcher takes picks by rank (R6Args.no_runs == 0), with descriptor ids from a helper's slots
                for (u32 g0 = 128u; g0 + 8u <= did; g0 += 64u) {
                    bool run = true;
                    for (u32 q = 0; q < 8u; ++q) run = run && tmpl[before + g0 + q] == tmpl[before + g0] && em.out[before + g0 + q] >= 0;
                    if (run) ++late_run_groups;
                }
                if (blk.cut_exception != ce_before && did == 1u) ++late_exception_first;   // (the block's first task from its exception list: thread 0's record)
                if (blk.cut_uncounted != cu_before && did >= 129u) ++late_cut_uncounted;
                for (u32 k = ninf_before; k < em.ctl.ninf; ++k)
                    if (em.inf_task[k] - before >= 128u) ++late_unplaceable;
                if (did > 15u * 64u) ++rounds_two_groups;                     // a helper wave applied a second group
                if (did >= 15u * 64u && did < cnt_round) ++cuts_late;         // the block was cut inside a group >= 15
                if (blk.cut_window != wc_before) {
                    // the task the window ran out for is the next round's first: that round must decide it (checked when it ends)
                    pending_cut = blk.pos;
                }
                if (pending_seen != R6_NONE && blk.pos > pending_seen) {   // the round behind a window cut decided the task: as the model does?
                    if (em.out[pending_seen] != ref.out[pending_seen]) { fprintf(stderr, "task %u behind a window cut: node %d, model %d\n", pending_seen, em.out[pending_seen], ref.out[pending_seen]); return false; }
                    ++window_cut_then_decided;
                    pending_seen = R6_NONE;
                }
                if (pending_cut != R6_NONE) { pending_seen = pending_cut; pending_cut = R6_NONE; }
            }
            ++rounds;
            if (blk.error) { fprintf(stderr, "kernel reported error %u at task %u\n", blk.error, blk.pos); return false; }
            if (blk.pos <= before) { fprintf(stderr, "no progress at task %u\n", before); return false; }
        }
        // one more round past the end must be a no-op
        if (compact) {
            grid(1, 1024, 256, [a]() { k_r6_compact(a); });
            grid(B, 64 * R6_PW, r6_propose_lds(p.Wn), [a]() { k_r6_propose_c(a); });
            grid(1, R6_COMMIT_THREADS, r6_commit_lds(p.Wn, B, n_dc + n_dm, true, arg_win), [a]() { k_r6_commit_c(a); });
        } else {
            propose_plain();
            if (mounts) grid(1, R6_COMMIT_THREADS, r6_commit_lds(p.Wn, B, n_dc + n_dm, false, arg_win), [a]() { k_r6_commit_v(a); });
            else grid(1, R6_COMMIT_THREADS, r6_commit_lds(p.Wn, B, n_dc + n_dm, false, arg_win), [a]() { k_r6_commit(a); });
        }
        return blk.pos == j1;
    };
    bool ok = split ? (stretch(0, T / 3) && stretch(T / 3, T)) : stretch(0, T);
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
    if (mounts) {   // the attachment rows of every task with mounts, the final usage of every volume
        ok = ok && same("att", att, mr.att, mr.csi_set.size() * VOL_MAX_MOUNTS);
        for (u32 v = 0; ok && v < vp.vol.size(); ++v) {
            const VolDyn want = vp.derive(mr.use, v), d = vt.vdyn[v];
            if (d.n_tasks != want.n_tasks || d.n_writers != want.n_writers || (want.n_tasks && d.pin != want.pin)) {
                fprintf(stderr, "MISMATCH usage of volume %u: emu {%u tasks, %u writers, pin %08x} model {%u, %u, %08x}\n", v, d.n_tasks, d.n_writers, d.pin, want.n_tasks, want.n_writers, want.pin);
                ok = false;
            }
        }
        u64 pin_on = 0, pin_failed = 0, pin_elsewhere = 0;   // the tasks after the pinned single-node volume: on its node, or nowhere
        for (u32 j = 0; hot && j < T; ++j)
            if (mr.is(j) && mr.csi_set[mr.csi_of[j]] <= 6) (ref.out[j] == (int32_t)N - 1 ? pin_on : ref.out[j] < 0 ? pin_failed : pin_elsewhere)++;
        fprintf(stderr, "reach mounts: tasks=%zu with_attachments=%llu failed_choice=%llu no_node=%llu cut_at_second_mount=%llu pinned_on_node=%llu pinned_unplaced=%llu pinned_elsewhere=%llu\n",
                mr.csi_set.size(), (unsigned long long)mr.with_att, (unsigned long long)mr.failed_choice, (unsigned long long)mr.no_node, (unsigned long long)cut_at_mount,
                (unsigned long long)pin_on, (unsigned long long)pin_failed, (unsigned long long)pin_elsewhere);
    }
    // the incrementally maintained bitmaps against a rebuild from the final node rows (same base: levels are relative to it)
    if (ok) {
        std::vector<u64> planes2 = planes, rr2 = rr, rg2 = rg;
        const u32 base = blk.base, maxrel = blk.maxrel;
        grid((p.Wn + 3) / 4, 256, 0, [a]() { k_r6_rows(a); });
        ok = same("planes", planes2, planes, planes.size()) && same("rr", rr2, rr, (size_t)(n_dc + n_dm) * p.Wn) && same("rg", rg2, rg, p.rg_kind.size() * p.Wn);
        u32 hi = 0;
        for (u32 n = 0; n < N; ++n)
            if ((p.valid[n >> 6] >> (n & 63)) & 1) hi = std::max(hi, em.total[n] - base);
        if (maxrel < hi) { fprintf(stderr, "maxrel %u below the highest level %u\n", maxrel, hi); ok = false; }
    }
    if (verbose || !ok)
        fprintf(stderr, "seed %u N %u T %u S %u block %u order %d feat %d split %d: placed %u inf %u | rounds %llu (%.1f tasks each) cut: exhausted %u exception %u uncounted %u | compact rounds %u | classes %u+%u -> %s\n",
                seed, N, T, S, B, order, feat, (int)split, em.ctl.ncommit, em.ctl.ninf, (unsigned long long)rounds, rounds ? (double)T / (double)rounds : 0.0, blk.cut_exhausted,
                blk.cut_exception, blk.cut_uncounted, blk.crounds, n_dc, n_dm, ok ? "OK" : "FAIL");
    fprintf(stderr, "reach window: win=%u block=%u rounds=%llu long_lists=%llu longest=%llu rounds_two_groups=%llu cuts_late=%llu window_cuts=%u window_cut_then_decided=%llu cut_exhausted=%u compact_rounds=%u ext=%u\n",
            dbg_win ? std::min<u32>(dbg_win, r6_win_of(arg_win)) : r6_win_of(arg_win), B, (unsigned long long)rounds, (unsigned long long)long_lists, (unsigned long long)longest, (unsigned long long)rounds_two_groups,
            (unsigned long long)cuts_late, blk.cut_window, (unsigned long long)window_cut_then_decided, blk.cut_exhausted, blk.crounds, no_ext ? 0u : 1u);
    fprintf(stderr, "reach heads: late_cut_exception=%llu late_cut_mount=%llu late_cut_uncounted=%llu late_unplaceable=%llu late_run_groups=%llu late_run_tasks=%u first_from_exception_list=%llu no_runs=%u timers=%u\n",
            (unsigned long long)late_cut_exception, (unsigned long long)late_cut_mount, (unsigned long long)late_cut_uncounted, (unsigned long long)late_unplaceable, (unsigned long long)late_run_groups, blk.dbg_late_runs,
            (unsigned long long)late_exception_first, no_runs ? 1u : 0u, timers ? 1u : 0u);
    if (compact && blk.crounds != crounds_checked) { fprintf(stderr, "compact rounds %u counted, %llu seen\n", blk.crounds, (unsigned long long)crounds_checked); return 1; }
    return ok ? 0 : 1;
}
