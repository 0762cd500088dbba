// emu_resolve6_levels.cpp — emu_resolve6_window.cpp's run of the block resolver's kernel source against the sequential model, with what
// LISTS OVER TWO LEVELS add (swp_resolve6.hpp, r6_propose_t "the second section", R6Args.levels2). Besides the outcome — placements,
// commit log, unplaceable records, node rows, bitmaps — every proposal of every round is compared with the list rule restated on the
// host from the state in front of the round: the first section's length, whether there is a second one, its entries one by one and
// bit 31. It REPORTS, on a "reach levels:" line, what a run came across, so that tests/test_emu_resolve6_levels.py asserts it instead of
// assuming it. TEST INFRASTRUCTURE; not product. Stand-alone: it is also built with -fsanitize=address,undefined.
//
//   emu_resolve6_levels <seed> <N> <T> <S> <block> <order: 0 rr | 1 major | 2 random> <features 0..4> [v] [t] [n] [m<k>] [a]
//       [l0: R6Args.levels2 = 0] [x: R6Args.ext == nullptr, lists of 2 * R6_CAND entries] [W<k>: a window of k entries through R6Args.dbg]
//       [P: R6Args.dbg bit 4 — the section timers, and with them Blk6.dbg_lv2] [R: one "round:" line per commit launch, for the
//       comparison of two builds]
//   emu_resolve6_levels fuzz <first seed> <count>     shapes drawn from the seed (N of 2 112 / 2 304 / 4 160, T <= 8 000, every order,
//                                                     features 0..4), each against the model and the restated rule
// Built with -DR6_LEVELS2=0 the kernels carry no second section at all: the build `l0` runs are compared with.
#include "wv_emu.hpp"

#include <tuple>

enum {
    R6R_ROUND, R6R_THREE_STOPS, R6R_IDLE_LANES, R6R_SECOND_STEP, R6R_AT_NENT, R6R_CLAMPED, R6R_ONE_ENTRY, R6R_SHORT_GROUP, R6R_FIRST_EXC,
    R6R_UNCOUNTED, R6R_MOUNTS, R6R_BEHIND_RUNS, R6R_COMPACT, R6R_R7, R6R_N
};
struct RoundRec { uint32_t pos, acc, why, seat_steps, reseats, rounds, total_reseats, cut_exhausted, cut_window, cut_exception, cut_uncounted; uint64_t picks; };
static std::vector<RoundRec> g_rounds;
static bool r6_reach_round(const void* blk, uint32_t pos, uint32_t acc, uint32_t why, uint32_t seat_steps, uint32_t reseats, const uint32_t* pk_node, const uint32_t* pk_idx, const uint32_t* pk_aux);
#define R6_REACH(what, cond)                       \
    do {                                           \
        if constexpr ((what) == R6R_ROUND) {       \
            (void)(cond);                          \
        }                                          \
    } while (0)

#define SWP_R6_KERNELS
#include "../../swarmkit_amd/csrc/swp_resolve6.hpp"

#include "emu_model.hpp"

static bool r6_reach_round(const void* blk, uint32_t pos, uint32_t acc, uint32_t why, uint32_t seat_steps, uint32_t reseats, const uint32_t* pk_node, const uint32_t* pk_idx, const uint32_t* pk_aux) {
    const Blk6* b = static_cast<const Blk6*>(blk);
    uint64_t h = 1469598103934665603ull;   // the pick slots of the accepted tasks, folded
    auto fold = [&](uint32_t v) { h = (h ^ v) * 1099511628211ull; };
    for (uint32_t i = 0; i < acc; ++i) { fold(pk_node[i]); fold(pk_idx[i]); fold(pk_aux[i]); }
    g_rounds.push_back(RoundRec{pos, acc, why, seat_steps, reseats, b->rounds, b->reseats, b->cut_exhausted, b->cut_window, b->cut_exception, b->cut_uncounted, h});
    return true;
}

template <class F>
static void grid(u32 blocks, u32 threads, size_t lds, F body) {
    for (u32 b = 0; b < blocks; ++b) {
        emu::blockidx() = b;
        emu::launch(threads, lds, body);
    }
    emu::blockidx() = 0;
}

struct Opt {
    bool verbose = false, task_rows = false, twins = true, adjacent = false, no_ext = false, levels = true, prof = false, records = false;
    u32 every = 10, dbg_win = 0;
};

// what a run came across
struct Reach {
    u64 rounds = 0, sections = 0, section_entries = 0, truncated = 0, crossed = 0, crossed_late = 0, no_room = 0, first_word = 0, beyond_maxrel = 0, twins_use_level = 0,
        nothing_in_front = 0, list_cut = 0, crossed_by_run = 0, cut_at_section = 0, cut_dry_section = 0, uncounted_before_section = 0, mounts_no_section = 0, sections_task_rows = 0, dbg_lv2 = 0, window_cuts = 0,
        cut_exhausted = 0;
};

static int run_case(u32 seed, u32 N, u32 T, u32 S, u32 B, int order, int feat, const Opt& o, Reach* reach_out) {
    const bool mounts = feat >= 4;
    Problem p = make_problem(seed, N, T, S, order, feat);
    VolProblem vp;
    MountRun mr;
    VolTables vt;
    if (mounts) {
        vp = make_volumes(seed, N, 8, 30, 0);
        mr = make_mounts(vp, seed, T, o.every, o.adjacent, 0, false, false);
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
    if (o.task_rows) n_dc = n_dm = 0;

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
    a.ext = o.no_ext ? nullptr : ext.data();
    a.dbg = (o.dbg_win << 12) | (o.prof ? 16u : 0u);
    a.levels2 = o.levels ? 1u : 0u;
    std::vector<u64> trows((size_t)B * p.Wn, 0x7777777777777777ull);
    a.task_rows = o.task_rows ? 1u : 0u;
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
    // identical tasks: the first task with the same record (but for its list slot) and generic set
    std::vector<u32> tmpl(T);
    {
        std::map<std::tuple<u32, u32, u32, i64, i64, u32, u64, u32, u32>, u32> first;
        for (u32 j = 0; j < T; ++j) {
            const RTask& r = p.rt[j];
            tmpl[j] = first.emplace(std::make_tuple(r.svc, r.sc, r.flags, r.cpu, r.mem, r.pset, r.maxrep, p.tg.empty() ? 0u : p.tg[j], mounts && mr.is(j) ? mr.csi_set[mr.csi_of[j]] : 0u), j).first->second;
        }
    }
    a.tmpl = o.twins ? tmpl.data() : nullptr;

    Reach rc;
    const u32 lmax = o.no_ext ? 2u * R6_CAND : (u32)R6_LIST;
    auto entry = [&](u32 j, u32 k, u32* hw, u32* hb) {
        if (k < 2u * R6_CAND) { *hw = prop[j].hw[k]; *hb = prop[j].hb[k]; }
        else { *hw = ext[j].hw[k - 2u * R6_CAND]; *hb = ext[j].hb[k - 2u * R6_CAND]; }
    };
    // The list rule restated from the state in front of a round (em is what the propose kernels read): per task of the block without
    // cluster mounts the first section's half-words and, where the rule allows one, the second section's.
    struct Want { bool plain = false, has2 = false, trunc2 = false; u32 level = 0, len1 = 0; std::vector<std::pair<u32, u32>> sec2; };
    std::vector<Want> want(B);
    auto restate = [&](u32 pos, u32 cnt, u32 maxrel_before) {
        std::vector<u64> Fr;
        scan_window(p, em, pos, cnt, Fr);
        std::map<u32, u32> seen;
        for (u32 j = 0; j < cnt; ++j) {
            Want& w = want[j];
            w = Want{};
            const u32 gj = pos + j;
            const RTask& r = p.rt[gj];
            const u32 twins = o.twins ? seen[tmpl[gj]]++ : 0u;
            if (mounts && mr.is(gj)) continue;   // (its candidates depend on the volumes as they stand: only "no second section" is checked)
            std::vector<u32> cand;
            u32 L = 0xFFFFFFFFu;
            for (u32 n = 0; n < N; ++n) {
                if (!((Fr[(size_t)j * p.Wn + (n >> 6)] >> (n & 63)) & 1)) continue;
                if ((em.X[(size_t)r.svc * p.Wn + (n >> 6)] >> (n & 63)) & 1) continue;
                cand.push_back(n);
                L = std::min(L, em.total[n]);
            }
            if (cand.empty()) continue;
            w.plain = true;
            w.level = L;
            std::vector<u32> onL, onL1;
            for (u32 n : cand) {
                if (em.total[n] == L) onL.push_back(n);
                if (em.total[n] == L + 1) onL1.push_back(n);
            }
            const u32 h0 = onL[0] / 32u;
            if (twins >= onL.size()) { w.len1 = 1; ++rc.twins_use_level; continue; }   // the level's last half-word: a cut
            // half-words whose candidates all lie among the first `twins` are passed over
            std::vector<u32> hws;
            for (size_t i = 0; i < onL.size(); ++i) {
                const u32 h = onL[i] / 32u;
                size_t last = i;
                while (last + 1 < onL.size() && onL[last + 1] / 32u == h) ++last;
                if (last >= twins) hws.push_back(h);
                i = last;
            }
            w.len1 = (u32)std::min<size_t>(hws.size(), lmax);
            if (hws.size() > lmax) { ++rc.list_cut; continue; }
            if (!o.levels || !R6_LEVELS2) continue;
            if (hws.size() == lmax) { ++rc.no_room; continue; }
            if (L + 1 - blk.base > maxrel_before) { ++rc.beyond_maxrel; continue; }
            if (h0 / 2u == 0) { ++rc.first_word; continue; }
            std::vector<std::pair<u32, u32>> s2;   // (half-word, bits) of level L + 1 in the words in front of h0's
            for (u32 n : onL1) {
                if (n / 64u >= h0 / 2u) break;
                if (s2.empty() || s2.back().first != n / 32u) s2.push_back({n / 32u, 0u});
                s2.back().second |= 1u << (n & 31u);
            }
            if (s2.empty()) { ++rc.nothing_in_front; continue; }
            const u32 room = lmax - w.len1;
            w.trunc2 = s2.size() > room;
            if (s2.size() > room) s2.resize(room);
            w.has2 = true;
            w.sec2 = s2;
        }
    };
    auto check_proposals = [&](u32 pos, u32 cnt) -> bool {
        for (u32 j = 0; j < cnt; ++j) {
            const u32 gj = pos + j;
            const bool is_mount = mounts && mr.is(gj);
            const u32 nc = prop[j].level != R6_NONE ? (prop[j].n_cand & 0x7FFFFFFFu) : 0u;
            if (nc > lmax) { fprintf(stderr, "task %u: a list of %u entries\n", gj, nc); return false; }
            u32 brk = nc;   // the first entry whose half-word does not ascend: where a second section starts
            for (u32 k = 1; k < nc; ++k) {
                u32 h0_, b0_, h1_, b1_;
                entry(j, k - 1, &h0_, &b0_);
                entry(j, k, &h1_, &b1_);
                if (h1_ <= h0_) { brk = k; break; }
            }
            if (is_mount) {
                if (brk != nc) { fprintf(stderr, "task %u has cluster mounts and a second section\n", gj); return false; }
                if (nc) ++rc.mounts_no_section;
                continue;
            }
            const Want& w = want[j];
            if (w.plain != (prop[j].level != R6_NONE)) { fprintf(stderr, "task %u: plain candidates: kernel %d, restated %d\n", gj, prop[j].level != R6_NONE, (int)w.plain); return false; }
            if (!w.plain) continue;
            if (prop[j].level != w.level) { fprintf(stderr, "task %u: level %u, restated %u\n", gj, prop[j].level, w.level); return false; }
            const u32 len2 = w.has2 ? (u32)w.sec2.size() : 0u;
            if (brk != (len2 ? w.len1 : nc) || nc != w.len1 + len2) {
                fprintf(stderr, "task %u: list of %u entries, second section at %u; restated %u + %u\n", gj, nc, brk, w.len1, len2);
                return false;
            }
            for (u32 k = 0; k < len2; ++k) {
                u32 hw, hb;
                entry(j, w.len1 + k, &hw, &hb);
                if (hw != w.sec2[k].first || hb != w.sec2[k].second) {
                    fprintf(stderr, "task %u: entry %u of the second section is (%u, %08x), restated (%u, %08x)\n", gj, k, hw, hb, w.sec2[k].first, w.sec2[k].second);
                    return false;
                }
            }
            if (len2) {
                if (((prop[j].n_cand >> 31) != 0) != w.trunc2) { fprintf(stderr, "task %u: bit 31 is %u, the second section was%s cut by the room\n", gj, prop[j].n_cand >> 31, w.trunc2 ? "" : " not"); return false; }
                ++rc.sections;
                rc.section_entries += len2;
                if (w.trunc2) ++rc.truncated;
                if (o.task_rows) ++rc.sections_task_rows;
            }
        }
        return true;
    };

    auto build = [&]() {
        grid(1, 1024, 256, [a]() { k_r6_minmax(a); });
        grid((p.Wn + 3) / 4, 256, 0, [a]() { k_r6_rows(a); });
    };
    auto propose_plain = [&]() {   // the instance launch_r6_rounds picks for the node set
        if (p.Wn <= R6_TINY_WORDS && B > 1024u) grid(B, 64 * R6_PW_TINY, r6_propose_lds(p.Wn), [a]() { k_r6_propose_tiny(a); });
        else if (p.Wn <= R6_SMALL_WORDS) grid(B, 64 * R6_PW, r6_propose_lds(p.Wn), [a]() { k_r6_propose_small(a); });
        else grid(B, 64 * R6_PW, r6_propose_lds(p.Wn), [a]() { k_r6_propose(a); });
    };
    auto commit = [&]() {
        if (mounts) grid(1, R6_COMMIT_THREADS, r6_commit_lds(p.Wn, B, n_dc + n_dm, false, 0), [a]() { k_r6_commit_v(a); });
        else grid(1, R6_COMMIT_THREADS, r6_commit_lds(p.Wn, B, n_dc + n_dm, false, 0), [a]() { k_r6_commit(a); });
    };
    build();
    if (blk.error) { fprintf(stderr, "build reported error %u\n", blk.error); return 3; }
    blk.pos = 0;
    blk.end = T;
    while (blk.pos < blk.end) {
        const u32 before = blk.pos, cnt_round = std::min(B, blk.end - blk.pos);
        for (R6Prop& q : prop) memset(&q, 0xEE, sizeof q);
        for (R6PropExt& q : ext) memset(&q, 0xEE, sizeof q);
        const u32 ce = blk.cut_exhausted, cw = blk.cut_window, cu = blk.cut_uncounted, maxrel_before = blk.maxrel;
        if (o.task_rows)
            for (u32 gy = 0; gy < (B + 63) / 64; ++gy) {   // grid (words / 4, groups of the block)
                emu::blockidx_y() = gy;
                grid((p.Wn + 3) / 4, 256, (size_t)B * 16, [a]() { k_r6_taskrows(a); });
            }
        emu::blockidx_y() = 0;
        if (mounts) {
            for (u32 by = 0; by < B; ++by) {   // grid (words / 256, block)
                emu::blockidx_y() = by;
                grid((p.Wn + 255) / 256, 256, 0, [a]() { k_r6_volrows(a); });
            }
            emu::blockidx_y() = 0;
        }
        restate(before, cnt_round, maxrel_before);
        propose_plain();
        if (!check_proposals(before, cnt_round)) return 3;
        const std::vector<u32> total_before = em.total;
        commit();
        const u32 did = blk.pos - before;
        for (u32 j = 0; j < did; ++j) {   // a task placed on a node that stood one level above its record's
            const int32_t nd = em.out[before + j];
            if (nd < 0 || prop[j].level == R6_NONE) continue;
            if (total_before[(u32)nd] == prop[j].level + 1u) {
                // (without a section of its own: the runs-by-rank path gave it the next free candidate of the list of its run's first task — an
                // identical task, whose second section is this task's as well; only with the twins' ids, and the model decides whether it was right)
                if (!want[j].has2 && !o.twins) { fprintf(stderr, "task %u took node %d one level up without a second section\n", before + j, nd); return 3; }
                if (!want[j].has2) ++rc.crossed_by_run;
                ++rc.crossed;
                if (j >= 128u) ++rc.crossed_late;   // (group >= 2: a helper staged its window)
            } else if (total_before[(u32)nd] != prop[j].level) {
                fprintf(stderr, "task %u took node %d on level %u, its record says %u\n", before + j, nd, total_before[(u32)nd], prop[j].level);
                return 3;
            }
        }
        if (did < cnt_round && (blk.cut_exhausted != ce || blk.cut_window != cw) && want[did].has2) ++rc.cut_at_section;
        if (did < cnt_round && blk.cut_exhausted != ce) {
            // cut with the reason "exhausted": every entry of the task's list, first and second section alike, must name only nodes this
            // round's tasks in front of it took — a live entry would make the cut a wrong one. With a second section: the case is counted.
            std::vector<bool> took(N, false);
            for (u32 j = 0; j < did; ++j)
                if (em.out[before + j] >= 0) took[(u32)em.out[before + j]] = true;
            const u32 nc = prop[did].level != R6_NONE ? (prop[did].n_cand & 0x7FFFFFFFu) : 0u;
            for (u32 k = 0; k < nc; ++k) {
                u32 hw, hb;
                entry(did, k, &hw, &hb);
                for (u32 b = 0; b < 32; ++b)
                    if (((hb >> b) & 1u) && !took[hw * 32u + b]) { fprintf(stderr, "task %u: cut at an exhausted list, but node %u of entry %u is free\n", before + did, hw * 32u + b, k); return 3; }
            }
            if (want[did].has2) ++rc.cut_dry_section;
        }
        if (blk.cut_uncounted != cu)
            for (u32 j = did; j < cnt_round; ++j)
                if (want[j].has2) { ++rc.uncounted_before_section; break; }
        ++rc.rounds;
        if (blk.error) { fprintf(stderr, "kernel reported error %u at task %u\n", blk.error, blk.pos); return 3; }
        if (blk.pos <= before) { fprintf(stderr, "no progress at task %u\n", before); return 3; }
    }
    propose_plain();   // one more round past the end must be a no-op
    commit();
    if (blk.pos != T) return 3;
    rc.dbg_lv2 = blk.dbg_lv2;
    rc.window_cuts = blk.cut_window;
    rc.cut_exhausted = blk.cut_exhausted;
    if (o.prof && blk.dbg_lv2 != rc.sections) { fprintf(stderr, "Blk6.dbg_lv2 %u, %llu second sections seen\n", blk.dbg_lv2, (unsigned long long)rc.sections); return 1; }
    if (!o.prof && blk.dbg_lv2 != 0) { fprintf(stderr, "Blk6.dbg_lv2 counted without the timers' bit\n"); return 1; }

    bool ok = same("out", em.out, ref.out, T) && same("cpu", em.cpu, ref.cpu, N) && same("mem", em.mem, ref.mem, N) && same("total", em.total, ref.total, N) &&
              same("X", em.X, ref.X, em.X.size()) && same("portmap", em.portmap, ref.portmap, em.portmap.size()) &&
              same("list_node", em.list_node, ref.list_node, em.list_node.size()) && same("list_svc", em.list_svc, ref.list_svc, em.list_svc.size()) &&
              same("list_fail", em.list_fail, ref.list_fail, em.list_fail.size()) && same("gcnt", em.gcnt, ref.gcnt, em.gcnt.size());
    ok = ok && em.ctl.ncommit == ref.ctl.ncommit && em.ctl.ninf == ref.ctl.ninf;
    if (!ok) fprintf(stderr, "ncommit emu %u ref %u, ninf emu %u ref %u\n", em.ctl.ncommit, ref.ctl.ncommit, em.ctl.ninf, ref.ctl.ninf);
    ok = ok && same("log_node", em.log_node, ref.log_node, ref.ctl.ncommit) && same("log_task", em.log_task, ref.log_task, ref.ctl.ncommit) &&
         same("log_prev", em.log_prev, ref.log_prev, ref.ctl.ncommit) && same("last", em.last, ref.last, N) &&
         same("inf_task", em.inf_task, ref.inf_task, ref.ctl.ninf) && same("inf_pos", em.inf_pos, ref.inf_pos, ref.ctl.ninf);
    if (mounts) ok = ok && same("att", att, mr.att, mr.csi_set.size() * VOL_MAX_MOUNTS);
    if (ok) {   // the incrementally maintained bitmaps against a rebuild from the final node rows (same base: levels are relative to it)
        std::vector<u64> planes2 = planes, rr2 = rr, rg2 = rg;
        grid((p.Wn + 3) / 4, 256, 0, [a]() { k_r6_rows(a); });
        ok = same("planes", planes2, planes, planes.size()) && same("rr", rr2, rr, (size_t)(n_dc + n_dm) * p.Wn) && same("rg", rg2, rg, p.rg_kind.size() * p.Wn);
    }
    if (o.verbose || !ok)
        fprintf(stderr, "seed %u N %u T %u S %u block %u order %d feat %d levels2 %u: placed %u inf %u | rounds %llu (%.1f tasks each) cut: exhausted %u window %u exception %u uncounted %u -> %s\n", seed, N, T,
                S, B, order, feat, a.levels2, em.ctl.ncommit, em.ctl.ninf, (unsigned long long)rc.rounds, rc.rounds ? (double)T / (double)rc.rounds : 0.0, blk.cut_exhausted, blk.cut_window,
                blk.cut_exception, blk.cut_uncounted, ok ? "OK" : "FAIL");
    *reach_out = rc;
    return ok ? 0 : 1;
}

static void print_reach(const Reach& r, u32 levels2, u32 lmax) {
    fprintf(stderr,
            "reach levels: levels2=%u list=%u rounds=%llu sections=%llu section_entries=%llu truncated=%llu crossed=%llu crossed_in_late_group=%llu no_room=%llu first_word=%llu beyond_maxrel=%llu "
            "crossed_by_run=%llu twins_use_level=%llu nothing_in_front=%llu list_cut=%llu cut_at_section=%llu cut_dry_section=%llu uncounted_before_section=%llu mounts_no_section=%llu sections_task_rows=%llu dbg_lv2=%llu window_cuts=%llu "
            "cut_exhausted=%llu\n",
            levels2, lmax, (unsigned long long)r.rounds, (unsigned long long)r.sections, (unsigned long long)r.section_entries, (unsigned long long)r.truncated, (unsigned long long)r.crossed,
            (unsigned long long)r.crossed_late, (unsigned long long)r.no_room, (unsigned long long)r.first_word, (unsigned long long)r.beyond_maxrel, (unsigned long long)r.crossed_by_run, (unsigned long long)r.twins_use_level,
            (unsigned long long)r.nothing_in_front, (unsigned long long)r.list_cut, (unsigned long long)r.cut_at_section, (unsigned long long)r.cut_dry_section, (unsigned long long)r.uncounted_before_section,
            (unsigned long long)r.mounts_no_section, (unsigned long long)r.sections_task_rows, (unsigned long long)r.dbg_lv2, (unsigned long long)r.window_cuts, (unsigned long long)r.cut_exhausted);
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "fuzz")) {
        const u32 first = (u32)atoi(argv[2]), count = (u32)atoi(argv[3]);
        static const u32 sizes[3] = {2112, 2304, 4160};
        Reach sum;
        u32 bad = 0;
        for (u32 seed = first; seed < first + count; ++seed) {
            std::mt19937_64 g(seed * 7919ull + 13);
            const int order = (int)(g() % 3), feat = (int)(g() % 5);
            // (heavy services, replica limits and uncounted tasks — features >= 1 — end rounds early, and a round proposes a whole block:
            // those batches stay short and their blocks small; a batch without them runs several laps in blocks of 1 408)
            const u32 N = sizes[g() % 3], T = feat >= 1 ? 400 + (u32)(g() % 801) : 2000 + (u32)(g() % 6001), S = 20 + (u32)(g() % 120), B = feat >= 1 ? ((g() % 2) ? 256u : 192u) : 1408u;
            Opt o;
            o.task_rows = g() % 6 == 0;
            o.no_ext = g() % 8 == 0;
            if (g() % 5 == 0) o.dbg_win = 4;
            Reach r;
            g_rounds.clear();
            const int rc = run_case(seed, N, T, S, B, order, feat, o, &r);
            printf("fuzz seed %u (N %u T %u S %u block %u order %d feat %d%s%s%s): rc %d, %llu rounds, %llu second sections, %llu tasks crossed\n", seed, N, T, S, B, order, feat, o.task_rows ? " t" : "",
                   o.no_ext ? " x" : "", o.dbg_win ? " W4" : "", rc, (unsigned long long)r.rounds, (unsigned long long)r.sections, (unsigned long long)r.crossed);
            fflush(stdout);
            if (rc) ++bad;
            sum.rounds += r.rounds;
            sum.sections += r.sections;
            sum.section_entries += r.section_entries;
            sum.truncated += r.truncated;
            sum.crossed += r.crossed;
            sum.crossed_late += r.crossed_late;
            sum.cut_at_section += r.cut_at_section;
            sum.cut_dry_section += r.cut_dry_section;
            sum.uncounted_before_section += r.uncounted_before_section;
            sum.mounts_no_section += r.mounts_no_section;
            sum.sections_task_rows += r.sections_task_rows;
        }
        print_reach(sum, 1, 0);
        printf("fuzz: %u seeds, %u failed\n", count, bad);
        return bad ? 1 : 0;
    }
    if (argc < 8) { fprintf(stderr, "usage: %s seed N T S block order features(0..4) [options] | fuzz first count\n", argv[0]); return 2; }
    const u32 seed = atoi(argv[1]), N = atoi(argv[2]), T = atoi(argv[3]), S = atoi(argv[4]), B = atoi(argv[5]);
    const int order = atoi(argv[6]), feat = atoi(argv[7]);
    Opt o;
    for (int i = 8; i < argc; ++i) {
        if (argv[i][0] == 'v') o.verbose = true;
        if (argv[i][0] == 't') o.task_rows = true;   // rows per task of the block, rebuilt every round, instead of demand-class rows
        if (argv[i][0] == 'n') o.twins = false;      // lists start at the level's first candidate (R6Args.tmpl == nullptr)
        if (argv[i][0] == 'm') o.every = std::max(atoi(argv[i] + 1), 1);
        if (argv[i][0] == 'a') o.adjacent = true;
        if (argv[i][0] == 'x') o.no_ext = true;
        if (argv[i][0] == 'l') o.levels = atoi(argv[i] + 1) != 0;
        if (argv[i][0] == 'P') o.prof = true;
        if (argv[i][0] == 'R') o.records = true;
        if (argv[i][0] == 'W') o.dbg_win = (u32)atoi(argv[i] + 1) & 31u;
    }
    Reach r;
    const int rc = run_case(seed, N, T, S, B, order, feat, o, &r);
    if (rc > 1) return rc;
    print_reach(r, o.levels && R6_LEVELS2 ? 1u : 0u, o.no_ext ? 2u * R6_CAND : (u32)R6_LIST);
    if (o.records)
        for (const RoundRec& q : g_rounds)
            printf("round: pos %u acc %u why %u seat_steps %u stops %u | rounds %u stops %u cut %u %u %u %u | picks %016llx\n", q.pos, q.acc, q.why, q.seat_steps, q.reseats, q.rounds, q.total_reseats,
                   q.cut_exhausted, q.cut_window, q.cut_exception, q.cut_uncounted, (unsigned long long)q.picks);
    return rc;
}
