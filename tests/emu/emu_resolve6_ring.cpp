// emu_resolve6_ring.cpp — the block resolver's RING rounds (swp_resolve6.hpp, R6Args.ring, k_r6_commit_r) on CPU fibers against the
// sequential model of emu_model.hpp: blocks longer than the commit kernel's ring of fifteen 64-task slots, so that slots are reused,
// with lists of up to R6_LIST_RING half-words. Checked: behind EVERY round the placements of the tasks it decided, at the end the whole
// state (placements, commit log, unplaceable records, node rows, bitmaps against a rebuild). It REPORTS, on a "reach ring:" line, what
// a run came across, so that tests/test_emu_resolve6_ring.py asserts the paths instead of assuming them.
// TEST INFRASTRUCTURE; not product. Stand-alone: it is also built with -fsanitize=address,undefined.
//
//   emu_resolve6_ring <seed> <N> <T> <S> <block> <order: 0 rr | 1 major | 2 random> <features 0..3> [v] [r0: flat rounds, R6Args.ring = 0]
//       [l0: R6Args.levels2 = 0] [W<k>: a window of k entries through R6Args.dbg] [t: task rows] [n: no twins]
//       [R: one "round:" line per FLAT commit launch, for the comparison of two builds]
//       [U<k>: every k-th task is uncounted] [E<j>: task j must use its exception list]
//   emu_resolve6_ring fuzz <first seed> <count>     shapes drawn from the seed, each against the model
// Built with -DR6_RING_ON=0 the kernels carry no ring at all: the build `r0` runs are compared with.
#include "wv_emu.hpp"

#include <tuple>

enum {
    R6R_ROUND, R6R_THREE_STOPS, R6R_IDLE_LANES, R6R_SECOND_STEP, R6R_AT_NENT, R6R_CLAMPED, R6R_ONE_ENTRY, R6R_SHORT_GROUP, R6R_FIRST_EXC,
    R6R_UNCOUNTED, R6R_MOUNTS, R6R_BEHIND_RUNS, R6R_COMPACT, R6R_R7, R6R_N
};
struct RoundRec { uint32_t pos, acc, why, seat_steps, reseats, rounds, total_reseats, cut_exhausted, cut_window, cut_exception, cut_uncounted; uint64_t picks; };
static std::vector<RoundRec> g_rounds;
static uint64_t g_reach[R6R_N], g_ring_reach[8];
static bool r6_reach_round(const void* blk, uint32_t pos, uint32_t acc, uint32_t why, uint32_t seat_steps, uint32_t reseats, const uint32_t* pk_node, const uint32_t* pk_idx, const uint32_t* pk_aux);
#define R6_REACH(what, cond)                       \
    do {                                           \
        if constexpr ((what) == R6R_ROUND) {       \
            (void)(cond);                          \
        } else if (cond)                           \
            ++g_reach[what];                       \
    } while (0)
#define R6_RING_REACH(what, cond) \
    do {                          \
        if (cond) ++g_ring_reach[what]; \
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
    bool verbose = false, ring = true, levels = true, task_rows = false, twins = true, records = false;
    u32 dbg_win = 0, uncounted_every = 0, exc_task = 0;
};

// what a run came across
struct Reach {
    u64 rounds = 0, slot_reused = 0, slots_reused_twice = 0, wrapped_stages = 0, skipped3 = 0, picked_ge64 = 0, picked_ge32 = 0, long_lists = 0, long_sections = 0, short_last_group = 0,
        cut_exhausted_wrapped = 0, cut_window_wrapped = 0, cut_uncounted_wrapped = 0, cut_exception_wrapped = 0, first_exc = 0, inf_wrapped = 0, crossed_wrapped = 0, cut_exhausted = 0, cut_window = 0;
    void add(const Reach& o) {
        const u64* s = &o.rounds;
        u64* d = &rounds;
        for (size_t i = 0; i < sizeof(Reach) / sizeof(u64); ++i) d[i] += s[i];
    }
};

static int run_case(u32 seed, u32 N, u32 T, u32 S, u32 B, int order, int feat, const Opt& o, Reach* reach_out) {
    if (feat > 3) { fprintf(stderr, "a batch with cluster mounts has no ring rounds (k_r6_commit_v)\n"); return 2; }
    if (o.ring && (!R6_RING_ON || B > R6_BMAX || B % 64u)) { fprintf(stderr, "a ring block is a multiple of 64 up to %u (and needs a build with the ring)\n", (u32)R6_BMAX); return 2; }
    Problem p = make_problem(seed, N, T, S, order, feat);
    if (o.uncounted_every)   // (U<k>: every k-th task does not count on its node — the block ends behind it, deep inside a long block)
        for (u32 j = o.uncounted_every - 1u; j < T; j += o.uncounted_every) p.rt[j].flags |= RT_UNCOUNTED;
    if (o.exc_task && o.exc_task < T) {
        // E<j>: task j becomes the one task of a service of its own that already runs on EVERY valid node (X all ones, an exception-list
        // entry per node): no plain candidate, so it must use its exception list — the block is cut in front of it, deep inside a long
        // block, and the next round starts with it
        RTask& r = p.rt[o.exc_task];
        const u32 s_new = p.S++;
        p.X.insert(p.X.end(), p.Wn, ~0ull);
        for (u32 n = 0; n < N; ++n)
            if ((p.valid[n >> 6] >> (n & 63)) & 1) {
                p.list_node.push_back(n);
                p.list_svc.push_back(1 + n % 3);
                p.list_fail.push_back(0);
            }
        r.svc = s_new;
        r.sc = 0;
        r.flags = 0;
        r.cpu = r.mem = 0;
        r.pset = 0;
        r.maxrep = 0;
        r.slot = (u32)p.list_node.size();
        p.list_node.push_back(LIST_EMPTY);
        p.list_svc.push_back(0);
        p.list_fail.push_back(0);
        p.list_off.push_back((u32)p.list_node.size());
        if (!p.tg.empty()) p.tg[o.exc_task] = 0;
    }
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
    ref_window(p, ref, 0, T, F, nullptr);

    std::vector<u64> planes((size_t)R6_NP * p.Wn, 0xAAAAAAAAAAAAAAAAull), rr((size_t)std::max<u32>(n_dc + n_dm, 1) * p.Wn, 0x5555555555555555ull);
    std::vector<R6Prop> prop(B);
    std::vector<R6PropExtRing> ext(B);   // room for either record: a ring round's R6PropExtRing, a flat round's R6PropExt at the buffer's front
    R6PropExt* const ext_flat = reinterpret_cast<R6PropExt*>(ext.data());
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
    a.ext = ext_flat;
    a.dbg = o.dbg_win << 12;
    a.levels2 = o.levels ? 1u : 0u;
    a.no_runs = o.ring ? 1u : 0u;   // (the ring instance has no runs-by-rank path whatever this says; flat rounds keep theirs)
#if R6_RING_ON
    a.ring = o.ring ? (u32)R6_RING : 0u;
#endif
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
    std::vector<u32> tmpl(T);
    {
        std::map<std::tuple<u32, u32, u32, i64, i64, u32, u64, u32>, u32> first;
        for (u32 j = 0; j < T; ++j) {
            const RTask& r = p.rt[j];
            tmpl[j] = first.emplace(std::make_tuple(r.svc, r.sc, r.flags, r.cpu, r.mem, r.pset, r.maxrep, p.tg.empty() ? 0u : p.tg[j]), j).first->second;
        }
    }
    a.tmpl = o.twins ? tmpl.data() : nullptr;

    Reach rc;
    const u32 ring = o.ring ? (u32)R6_RING : 0u;
    const u32 lmax = o.ring ? (u32)R6_LIST_RING : (u32)R6_LIST;
    auto entry = [&](u32 j, u32 k, u32* hw, u32* hb) {
        if (k < 2u * R6_CAND) { *hw = prop[j].hw[k]; *hb = prop[j].hb[k]; }
        else if (ring) { *hw = ext[j].hw[k - 2u * R6_CAND]; *hb = ext[j].hb[k - 2u * R6_CAND]; }
        else { *hw = ext_flat[j].hw[k - 2u * R6_CAND]; *hb = ext_flat[j].hb[k - 2u * R6_CAND]; }
    };
    auto build = [&]() {
        grid(1, 1024, 256, [a]() { k_r6_minmax(a); });
        grid((p.Wn + 3) / 4, 256, 0, [a]() { k_r6_rows(a); });
    };
    auto propose_plain = [&]() {   // the instance launch_r6_rounds picks for the node set: the _r ones in a ring round
#if R6_RING_ON
        if (o.ring) {
            if (p.Wn <= R6_TINY_WORDS && B > 1024u) grid(B, 64 * R6_PW_TINY, r6_propose_lds(p.Wn), [a]() { k_r6_propose_tiny_r(a); });
            else if (p.Wn <= R6_SMALL_WORDS) grid(B, 64 * R6_PW, r6_propose_lds(p.Wn), [a]() { k_r6_propose_small_r(a); });
            else grid(B, 64 * R6_PW, r6_propose_lds(p.Wn), [a]() { k_r6_propose_r(a); });
            return;
        }
#endif
        if (p.Wn <= R6_TINY_WORDS && B > 1024u) grid(B, 64 * R6_PW_TINY, r6_propose_lds(p.Wn), [a]() { k_r6_propose_tiny(a); });
        else if (p.Wn <= R6_SMALL_WORDS) grid(B, 64 * R6_PW, r6_propose_lds(p.Wn), [a]() { k_r6_propose_small(a); });
        else grid(B, 64 * R6_PW, r6_propose_lds(p.Wn), [a]() { k_r6_propose(a); });
    };
    auto commit = [&]() {
#if R6_RING_ON
        if (o.ring) {
            grid(1, R6_COMMIT_THREADS, r6_commit_lds_ring(p.Wn, B, n_dc + n_dm, ring, 0), [a]() { k_r6_commit_r(a); });
            return;
        }
#endif
        grid(1, R6_COMMIT_THREADS, r6_commit_lds(p.Wn, B, n_dc + n_dm, false, 0), [a]() { k_r6_commit(a); });
    };
    build();
    if (blk.error) { fprintf(stderr, "build reported error %u\n", blk.error); return 3; }
    blk.pos = 0;
    blk.end = T;
    while (blk.pos < blk.end) {
        const u32 before = blk.pos, cnt_round = std::min(B, blk.end - blk.pos);
        for (R6Prop& q : prop) memset(&q, 0xEE, sizeof q);
        for (R6PropExtRing& q : ext) memset(&q, 0xEE, sizeof q);
        const u32 ce = blk.cut_exhausted, cw = blk.cut_window, cu = blk.cut_uncounted, cx = blk.cut_exception;
        const u64 first_exc_before = g_reach[R6R_FIRST_EXC];
        if (o.task_rows)
            for (u32 gy = 0; gy < (B + 63) / 64; ++gy) {   // grid (words / 4, groups of the block)
                emu::blockidx_y() = gy;
                grid((p.Wn + 3) / 4, 256, (size_t)B * 16, [a]() { k_r6_taskrows(a); });
            }
        emu::blockidx_y() = 0;
        propose_plain();
        for (u32 j = 0; j < cnt_round; ++j) {   // the lists as the propose kernels left them
            const u32 nc = prop[j].level != R6_NONE ? (prop[j].n_cand & 0x7FFFFFFFu) : 0u;
            if (nc > lmax) { fprintf(stderr, "task %u: a list of %u entries\n", before + j, nc); return 3; }
            if (nc > (u32)R6_LIST) {
                ++rc.long_lists;
                for (u32 k = 1; k < nc; ++k) {
                    u32 h0_, b0_, h1_, b1_;
                    entry(j, k - 1, &h0_, &b0_);
                    entry(j, k, &h1_, &b1_);
                    if (h1_ <= h0_) { ++rc.long_sections; break; }   // a second section in a list beyond R6_LIST entries
                }
            }
        }
        const std::vector<u32> total_before = em.total;
        commit();
        const u32 did = blk.pos - before;
        if (blk.error) { fprintf(stderr, "kernel reported error %u at task %u\n", blk.error, blk.pos); return 3; }
        if (did == 0 || did > cnt_round) { fprintf(stderr, "round at task %u decided %u of %u\n", before, did, cnt_round); return 3; }
        // the round's outcome: every task it decided, against the model's
        for (u32 j = 0; j < did; ++j)
            if (em.out[before + j] != ref.out[before + j]) {
                fprintf(stderr, "round %llu (tasks %u.., %u decided): task %u (group %u, slot %u) on node %d, the model says %d\n", (unsigned long long)rc.rounds, before, did, before + j, j / 64u,
                        ring ? j % ring : j, em.out[before + j], ref.out[before + j]);
                return 1;
            }
        for (u32 j = 0; j < did; ++j) {
            const int32_t nd = em.out[before + j];
            if (nd < 0) { if (ring && j >= ring) ++rc.inf_wrapped; continue; }
            if (prop[j].level == R6_NONE) continue;
            const u32 nc = prop[j].n_cand & 0x7FFFFFFFu;
            for (u32 k = 0; k < nc; ++k) {
                u32 hw, hb;
                entry(j, k, &hw, &hb);
                if (hw == (u32)nd / 32u && ((hb >> ((u32)nd & 31u)) & 1u)) {
                    if (k >= 64u) ++rc.picked_ge64;
                    if (k >= 32u) ++rc.picked_ge32;
                    break;
                }
            }
            if (ring && j >= ring && total_before[(u32)nd] == prop[j].level + 1u) ++rc.crossed_wrapped;
        }
        if (ring && did > ring) ++rc.slot_reused;            // picks of a group >= 15 were applied: out of a slot that held another group's before
        if (ring && did > 2u * ring) ++rc.slots_reused_twice;
        if (ring && did == cnt_round && cnt_round > ring && cnt_round % 64u) ++rc.short_last_group;
        if (ring && did < cnt_round && did >= ring) {          // a cut inside (or in front of) a group that lives in a reused slot
            if (blk.cut_exhausted != ce) ++rc.cut_exhausted_wrapped;
            if (blk.cut_window != cw) ++rc.cut_window_wrapped;
            if (blk.cut_exception != cx) ++rc.cut_exception_wrapped;
        }
        if (ring && blk.cut_uncounted != cu && did > ring) ++rc.cut_uncounted_wrapped;
        if (g_reach[R6R_FIRST_EXC] != first_exc_before) ++rc.first_exc;
        ++rc.rounds;
    }
    propose_plain();   // one more round past the end must be a no-op
    commit();
    if (blk.pos != T) return 3;
    rc.cut_exhausted = blk.cut_exhausted;
    rc.cut_window = blk.cut_window;
    rc.skipped3 = g_ring_reach[R6RR_SKIPPED3];
    rc.wrapped_stages = g_ring_reach[R6RR_WRAPPED_STAGE];

    bool ok = same("out", em.out, ref.out, T) && same("cpu", em.cpu, ref.cpu, N) && same("mem", em.mem, ref.mem, N) && same("total", em.total, ref.total, N) &&
              same("X", em.X, ref.X, em.X.size()) && same("portmap", em.portmap, ref.portmap, em.portmap.size()) &&
              same("list_node", em.list_node, ref.list_node, em.list_node.size()) && same("list_svc", em.list_svc, ref.list_svc, em.list_svc.size()) &&
              same("list_fail", em.list_fail, ref.list_fail, em.list_fail.size()) && same("gcnt", em.gcnt, ref.gcnt, em.gcnt.size());
    ok = ok && em.ctl.ncommit == ref.ctl.ncommit && em.ctl.ninf == ref.ctl.ninf;
    if (!ok) fprintf(stderr, "ncommit emu %u ref %u, ninf emu %u ref %u\n", em.ctl.ncommit, ref.ctl.ncommit, em.ctl.ninf, ref.ctl.ninf);
    ok = ok && same("log_node", em.log_node, ref.log_node, ref.ctl.ncommit) && same("log_task", em.log_task, ref.log_task, ref.ctl.ncommit) &&
         same("log_prev", em.log_prev, ref.log_prev, ref.ctl.ncommit) && same("last", em.last, ref.last, N) &&
         same("inf_task", em.inf_task, ref.inf_task, ref.ctl.ninf) && same("inf_pos", em.inf_pos, ref.inf_pos, ref.ctl.ninf);
    if (ok) {   // the incrementally maintained bitmaps against a rebuild from the final node rows (same base: levels are relative to it)
        std::vector<u64> planes2 = planes, rr2 = rr, rg2 = rg;
        grid((p.Wn + 3) / 4, 256, 0, [a]() { k_r6_rows(a); });
        ok = same("planes", planes2, planes, planes.size()) && same("rr", rr2, rr, (size_t)(n_dc + n_dm) * p.Wn) && same("rg", rg2, rg, p.rg_kind.size() * p.Wn);
    }
    if (o.verbose || !ok)
        fprintf(stderr, "seed %u N %u T %u S %u block %u ring %u order %d feat %d: placed %u inf %u | rounds %llu (%.1f tasks each) cut: exhausted %u window %u exception %u uncounted %u -> %s\n", seed, N, T, S, B,
                ring, order, feat, em.ctl.ncommit, em.ctl.ninf, (unsigned long long)rc.rounds, rc.rounds ? (double)T / (double)rc.rounds : 0.0, blk.cut_exhausted, blk.cut_window, blk.cut_exception,
                blk.cut_uncounted, ok ? "OK" : "FAIL");
    *reach_out = rc;
    return ok ? 0 : 1;
}

static void print_reach(const Reach& r, u32 ring, u32 lmax) {
    fprintf(stderr,
            "reach ring: ring=%u list=%u rounds=%llu slot_reused=%llu slots_reused_twice=%llu wrapped_stages=%llu skipped3=%llu picked_ge64=%llu picked_ge32=%llu long_lists=%llu long_sections=%llu "
            "short_last_group=%llu cut_exhausted_wrapped=%llu cut_window_wrapped=%llu cut_uncounted_wrapped=%llu cut_exception_wrapped=%llu first_exc=%llu inf_wrapped=%llu crossed_wrapped=%llu "
            "cut_exhausted=%llu cut_window=%llu\n",
            ring, lmax, (unsigned long long)r.rounds, (unsigned long long)r.slot_reused, (unsigned long long)r.slots_reused_twice, (unsigned long long)r.wrapped_stages, (unsigned long long)r.skipped3,
            (unsigned long long)r.picked_ge64, (unsigned long long)r.picked_ge32, (unsigned long long)r.long_lists, (unsigned long long)r.long_sections, (unsigned long long)r.short_last_group,
            (unsigned long long)r.cut_exhausted_wrapped, (unsigned long long)r.cut_window_wrapped, (unsigned long long)r.cut_uncounted_wrapped, (unsigned long long)r.cut_exception_wrapped,
            (unsigned long long)r.first_exc, (unsigned long long)r.inf_wrapped, (unsigned long long)r.crossed_wrapped, (unsigned long long)r.cut_exhausted, (unsigned long long)r.cut_window);
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "fuzz")) {
        const u32 first = (u32)atoi(argv[2]), count = (u32)atoi(argv[3]);
        static const u32 sizes[3] = {2112, 4160, 8256};
        static const u32 blocks[4] = {1088, 1984, 2816, 1472};
        Reach sum;
        u32 bad = 0;
        for (u32 seed = first; seed < first + count; ++seed) {
            std::mt19937_64 g(seed * 7919ull + 13);
            const int order = (int)(g() % 3), feat = (int)(g() % 4);
            // (features >= 1 end rounds early and a round proposes a whole block: those batches stay short)
            const u32 N = sizes[g() % 3], B = feat >= 1 ? 1088u : blocks[g() % 4], T = feat >= 1 ? 1200 + (u32)(g() % 600) : 3000 + (u32)(g() % 4000), S = 20 + (u32)(g() % 120);
            Opt o;
            o.task_rows = g() % 6 == 0;
            if (g() % 5 == 0) o.dbg_win = 4;
            o.twins = g() % 8 != 0;
            Reach r;
            memset(g_ring_reach, 0, sizeof g_ring_reach);
            const int rc = run_case(seed, N, T, S, B, order, feat, o, &r);
            printf("fuzz seed %u (N %u T %u S %u block %u order %d feat %d%s%s%s): rc %d, %llu rounds, %llu with a reused slot, %llu picks at entry >= 64\n", seed, N, T, S, B, order, feat, o.task_rows ? " t" : "",
                   o.twins ? "" : " n", o.dbg_win ? " W4" : "", rc, (unsigned long long)r.rounds, (unsigned long long)r.slot_reused, (unsigned long long)r.picked_ge64);
            fflush(stdout);
            if (rc) ++bad;
            sum.add(r);
        }
        print_reach(sum, (u32)R6_RING, (u32)R6_LIST_RING);
        printf("fuzz: %u seeds, %u failed\n", count, bad);
        return bad ? 1 : 0;
    }
    if (argc < 8) { fprintf(stderr, "usage: %s seed N T S block order features(0..3) [options] | fuzz first count\n", argv[0]); return 2; }
    const u32 seed = atoi(argv[1]), N = atoi(argv[2]), T = atoi(argv[3]), S = atoi(argv[4]), B = atoi(argv[5]);
    const int order = atoi(argv[6]), feat = atoi(argv[7]);
    Opt o;
    for (int i = 8; i < argc; ++i) {
        if (argv[i][0] == 'v') o.verbose = true;
        if (argv[i][0] == 'r') o.ring = atoi(argv[i] + 1) != 0;
        if (argv[i][0] == 'l') o.levels = atoi(argv[i] + 1) != 0;
        if (argv[i][0] == 't') o.task_rows = true;
        if (argv[i][0] == 'n') o.twins = false;
        if (argv[i][0] == 'R') o.records = true;
        if (argv[i][0] == 'W') o.dbg_win = (u32)atoi(argv[i] + 1) & 31u;
        if (argv[i][0] == 'U') o.uncounted_every = (u32)atoi(argv[i] + 1);
        if (argv[i][0] == 'E') o.exc_task = (u32)atoi(argv[i] + 1);
    }
    if (!R6_RING_ON) o.ring = false;
    Reach r;
    const int rc = run_case(seed, N, T, S, B, order, feat, o, &r);
    if (rc > 1) return rc;
    print_reach(r, o.ring ? (u32)R6_RING : 0u, o.ring ? (u32)R6_LIST_RING : (u32)R6_LIST);
    if (o.records)
        for (const RoundRec& q : g_rounds)
            printf("round: pos %u acc %u why %u seat_steps %u stops %u | rounds %u stops %u cut %u %u %u %u | picks %016llx\n", q.pos, q.acc, q.why, q.seat_steps, q.reseats, q.rounds, q.total_reseats,
                   q.cut_exhausted, q.cut_window, q.cut_exception, q.cut_uncounted, (unsigned long long)q.picks);
    return rc;
}
