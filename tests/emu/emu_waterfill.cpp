// emu_waterfill.cpp — runs k_waterfill (swarmkit_amd/csrc/swp_waterfill.hpp, unchanged) on CPU fibers (wv_emu.hpp) against a sequential
// model that places the run one task at a time. TEST INFRASTRUCTURE (tests/test_emu_waterfill.py).
//
// The kernel is written with raw HIP spellings; this translation unit supplies them: threadIdx.x is the current fiber, __shared__ is
// static storage (one workgroup of cooperative fibers), __syncthreads() is the harness's block barrier (a full barrier: the kernel's
// barriers order GLOBAL writes — ent[], cap[], ps[] —, which wv::barrier() on the device would not), the two wave shuffles are
// collectives of wv_emu.hpp.
//
//   emu_waterfill seeded <seed> <N> <len>   a drawn cluster state (task counts, residuals, exception lists with holes, failures below / at /
//                                           above MAX_FAILURES, non-zero commit and "no node" positions), five launches: services A B A C B.
//                                           len 0: runs of 1 and 2; 1: about one lap of the eligible nodes; 2: several laps; 3: more than the
//                                           cluster takes (reservations forced on, the tail finds no node)
//   emu_waterfill edge <name>               error | packed_below | packed_at | clamp | negzero | exactk
// Every mode prints a "reach waterfill:" line — what the MODEL's run came across —, then "-> OK" or the first difference.
#include "wv_emu.hpp"

// ---- the HIP spellings the kernel uses ------------------------------------------------------------------------------------------
#define __global__
#define __launch_bounds__(n)
#define __shared__ static
#define __forceinline__ inline
struct EmuThreadIdx {
    struct X {
        operator swpdev::u32() const { return wv::tid(); }
    } x;
};
static EmuThreadIdx threadIdx;
static inline void __syncthreads() { emu::block_barrier(); }
static inline swpdev::u64 __shfl_xor(swpdev::u64 v, int off, int width) {
    if (width != 64) abort();
    return wv::shfl_xor64(v, (swpdev::u32)off);
}
static inline int __shfl_up(int v, int off, int width) {
    if (width != 64) abort();
    return (int)(swpdev::u32)wv::shfl_up64((swpdev::u32)v, (swpdev::u32)off);
}
static inline swpdev::u64 atomicOr(swpdev::u64* p, swpdev::u64 v) {
    const swpdev::u64 old = *p;
    *p = old | v;
    return old;
}

#define SWP_WATERFILL_KERNEL
#include "../../swarmkit_amd/csrc/swp_waterfill.hpp"

#include <array>
#include <string>

#include "emu_model.hpp"

#define POISON 0xA5A5A5A5u
#define POISON64 0xA5A5A5A5A5A5A5A5ull

struct Run { u32 j0, count; };
struct WfCase {
    Problem p;                 // N, Wn, T, S, sc rows, rt, the lists, the node rows
    u32 xs = 0;                // stride of X: NOT n_words
    std::vector<Run> runs;
    u32 ncommit0 = 0, ninf0 = 0, error0 = ERR_NONE;
    std::vector<int32_t> last0;
};

struct Reach {   // counted by the model's run only
    u64 phases = 0, multi_count_phases = 0, entries_found = 0, entries_created = 0;
    u64 on_clean = 0, on_fail_below = 0, on_fail_at = 0, on_fail_above = 0, on_fail_only = 0, on_svc_positive = 0;
    u64 holes = 0, maxrep_cut = 0, negative_refused = 0, zero_vs_negative = 0, resource_refused = 0, exact_fit = 0;
    u64 tails = 0, none_eligible = 0, lapped_runs = 0, chain_continued = 0, tie_across_thread = 0, tie_across_wave = 0, huge_residual = 0;
    u64 list_reused = 0;   // a launch that found an entry an EARLIER launch of this case created
};

static State start_state(const WfCase& c) {
    const Problem& p = c.p;
    State s;
    s.cpu = p.cpu;
    s.mem = p.mem;
    s.total = p.total;
    s.X = p.X;
    s.list_node = p.list_node;
    s.list_svc = p.list_svc;
    s.list_fail = p.list_fail;
    s.out.assign(p.T + 8, -77);
    s.log_node.assign(c.ncommit0 + p.T + 8, POISON);
    s.log_task.assign(c.ncommit0 + p.T + 8, POISON);
    s.log_prev.assign(c.ncommit0 + p.T + 8, -7);
    s.last = c.last0;
    s.inf_task.assign(c.ninf0 + p.T + 8, POISON);
    s.inf_pos.assign(c.ninf0 + p.T + 8, POISON);
    memset(&s.ctl, 0x5A, sizeof s.ctl);   // every field the kernel must leave alone holds a pattern
    s.ctl.ncommit = c.ncommit0;
    s.ctl.ninf = c.ninf0;
    s.ctl.error = c.error0;
    return s;
}

// ---- the model: the reference's tick for a queue of identical tasks, one at a time (scheduler.go:694-748 with a heap of one; nodeLess
// :708-735; ResourceFilter.Check filter.go:77-84; MaxReplicasFilter.Check :373-375; NodeInfo.addTask nodeinfo.go:108-154). No phases,
// no capacities, no scans. skip_beyond: nodes whose entry does not fit k_waterfill's packed key are left out (what the KERNEL does with
// them, recorded by the "packed_at" edge); the true ranking has no such rule.
static void model_run(const WfCase& c, State& s, const Run& run, Reach& rc, bool skip_beyond, const std::vector<char>& made_before) {
    const Problem& p = c.p;
    if (s.ctl.error != ERR_NONE) return;
    const RTask& r0 = p.rt[run.j0];
    std::vector<u32> entry(p.N, LIST_EMPTY);   // the service's (node -> entry), as the reference's per-node maps have it
    for (u32 e = p.list_off[r0.svc]; e < p.list_off[r0.svc + 1]; ++e) {
        if (s.list_node[e] == LIST_EMPTY) { if (e < r0.slot) rc.holes++; continue; }
        entry[s.list_node[e]] = e;
    }
    const u32 C = (p.N + 1023) / 1024;   // (the kernel's thread geometry, for the tie counters only)
    std::vector<u32> served(p.N, 0);
    bool have_prev = false, tail = false;
    u64 prev_class = 0, prev_svc = 0, prev_total = 0;
    u32 prev_node = 0, distinct = 0;
    u32 placed = 0;
    bool any_eligible = false;
    for (u32 i = 0; i < run.count; ++i) {
        const u32 gj = run.j0 + i;
        const RTask& r = p.rt[gj];
        bool found = false;
        u64 b_class = 0, b_svc = 0, b_total = 0;
        u32 b_node = 0;
        for (u32 n = 0; n < p.N; ++n) {
            if (!((p.sc[(size_t)r.sc * p.Wn + (n >> 6)] >> (n & 63)) & 1)) continue;
            any_eligible = true;
            const u32 e = entry[n];
            const u64 svc = e == LIST_EMPTY ? 0 : s.list_svc[e], fails = e == LIST_EMPTY ? 0 : s.list_fail[e];
            if (r.flags & RT_RES) {
                if (r.cpu > s.cpu[n] || r.mem > s.mem[n]) {
                    if (i == 0) {
                        rc.resource_refused++;
                        if (s.cpu[n] < 0 || s.mem[n] < 0) rc.negative_refused++;
                        if ((r.cpu == 0 && s.cpu[n] < 0) || (r.mem == 0 && s.mem[n] < 0)) rc.zero_vs_negative++;
                    }
                    continue;
                }
                if ((r.cpu > 0 && r.cpu == s.cpu[n]) || (r.mem > 0 && r.mem == s.mem[n])) rc.exact_fit++;
                if (i == 0 && (s.cpu[n] >= (1ll << 61) || s.mem[n] >= (1ll << 61))) rc.huge_residual++;
            }
            if ((r.flags & RT_MAXREP) && svc >= r.maxrep) { if (i == 0 || served[n]) rc.maxrep_cut++; continue; }
            const u64 cls = fails >= MAX_FAILURES ? fails - (MAX_FAILURES - 1) : 0;
            if (skip_beyond && (svc >= (1ull << 24) || cls >= 255)) continue;
            const bool less = !found || cls < b_class || (cls == b_class && (svc < b_svc || (svc == b_svc && (s.total[n] < b_total || (s.total[n] == b_total && n < b_node)))));
            if (less) { found = true; b_class = cls; b_svc = svc; b_total = s.total[n]; b_node = n; }
        }
        if (!found) {   // no suitable node: recorded at the commit position of this moment
            s.inf_task[s.ctl.ninf] = gj;
            s.inf_pos[s.ctl.ninf] = s.ctl.ncommit;
            s.ctl.ninf++;
            tail = true;
            continue;
        }
        // reach: phases as stretches of one (class, svcCount); ties by index across the kernel's thread and wave borders
        if (!have_prev || prev_class != b_class || prev_svc != b_svc) {
            if (distinct > 1) rc.multi_count_phases++;
            rc.phases++;
            distinct = 1;
        } else if (b_total != prev_total)
            distinct++;
        else {
            if (prev_node / C != b_node / C) rc.tie_across_thread++;
            if (prev_node / C / 64 != b_node / C / 64) rc.tie_across_wave++;
        }
        have_prev = true;
        prev_class = b_class; prev_svc = b_svc; prev_total = b_total; prev_node = b_node;
        const u32 n = b_node, e = entry[n];
        if (e != LIST_EMPTY && !served[n]) {
            const u32 fl = s.list_fail[e];
            rc.entries_found++;
            if (made_before[e]) rc.list_reused++;
            if (s.list_svc[e] > 0) rc.on_svc_positive++;
            if (fl == 0) rc.on_clean++;
            else if (fl < MAX_FAILURES) rc.on_fail_below++;
            else if (fl == MAX_FAILURES) rc.on_fail_at++;
            else rc.on_fail_above++;
            if (fl && s.list_svc[e] == 0) rc.on_fail_only++;
        }
        // NodeInfo.addTask
        s.cpu[n] -= r.cpu;
        s.mem[n] -= r.mem;
        s.total[n] += 1;
        if (e == LIST_EMPTY) {
            s.X[(size_t)r.svc * c.xs + (n >> 6)] |= 1ull << (n & 63);
            s.list_node[r.slot] = n;
            s.list_svc[r.slot] = 1;
            s.list_fail[r.slot] = 0;
            entry[n] = r.slot;
            rc.entries_created++;
        } else
            s.list_svc[e] += 1;
        const u32 ci = s.ctl.ncommit++;
        s.log_node[ci] = n;
        s.log_task[ci] = gj;
        s.log_prev[ci] = s.last[n];
        if (s.last[n] >= 0 && (u32)s.last[n] < (u32)(ci - placed) ) rc.chain_continued++;
        s.last[n] = (int32_t)ci;
        s.out[gj] = (int32_t)n;
        served[n]++;
        ++placed;
    }
    if (distinct > 1) rc.multi_count_phases++;
    if (tail && placed) rc.tails++;
    if (!any_eligible) rc.none_eligible++;
    for (u32 n = 0; n < p.N; ++n)
        if (served[n] > 1) { rc.lapped_runs++; break; }
}

static void print_reach(const Reach& r, u64 true_model_differs) {
    fprintf(stderr,
            "reach waterfill: phases=%llu multi_count_phases=%llu entries_found=%llu entries_created=%llu on_clean=%llu on_fail_below=%llu on_fail_at=%llu on_fail_above=%llu on_fail_only=%llu "
            "on_svc_positive=%llu holes=%llu maxrep_cut=%llu negative_refused=%llu zero_vs_negative=%llu resource_refused=%llu exact_fit=%llu tails=%llu none_eligible=%llu lapped_runs=%llu "
            "chain_continued=%llu list_reused=%llu tie_across_thread=%llu tie_across_wave=%llu huge_residual=%llu true_model_differs=%llu\n",
            r.phases, r.multi_count_phases, r.entries_found, r.entries_created, r.on_clean, r.on_fail_below, r.on_fail_at, r.on_fail_above, r.on_fail_only, r.on_svc_positive, r.holes,
            r.maxrep_cut, r.negative_refused, r.zero_vs_negative, r.resource_refused, r.exact_fit, r.tails, r.none_eligible, r.lapped_runs, r.chain_continued, r.list_reused, r.tie_across_thread,
            r.tie_across_wave, r.huge_residual, true_model_differs);
}

// ---- every launch of the case on the kernel and on the model; every array the kernel can write compared in full after each one ------
static bool equal_states(const State& k, const State& m, u32 launch) {
    bool ok = same("out_node", k.out, m.out, m.out.size()) && same("cpu", k.cpu, m.cpu, m.cpu.size()) && same("mem", k.mem, m.mem, m.mem.size()) &&
              same("total", k.total, m.total, m.total.size()) && same("X", k.X, m.X, m.X.size()) && same("list_node", k.list_node, m.list_node, m.list_node.size()) &&
              same("list_svc", k.list_svc, m.list_svc, m.list_svc.size()) && same("list_fail", k.list_fail, m.list_fail, m.list_fail.size()) &&
              same("log_node", k.log_node, m.log_node, m.log_node.size()) && same("log_task", k.log_task, m.log_task, m.log_task.size()) &&
              same("log_prev", k.log_prev, m.log_prev, m.log_prev.size()) && same("last", k.last, m.last, m.last.size()) && same("inf_task", k.inf_task, m.inf_task, m.inf_task.size()) &&
              same("inf_pos", k.inf_pos, m.inf_pos, m.inf_pos.size());
    if (ok && (k.ctl.ncommit != m.ctl.ncommit || k.ctl.ninf != m.ctl.ninf || k.ctl.error != m.ctl.error)) {
        fprintf(stderr, "MISMATCH Ctl: emu {ncommit %u, ninf %u, error %u} model {%u, %u, %u}\n", k.ctl.ncommit, k.ctl.ninf, k.ctl.error, m.ctl.ncommit, m.ctl.ninf, m.ctl.error);
        ok = false;
    }
    if (ok && memcmp(&k.ctl, &m.ctl, sizeof(Ctl)) != 0) { fprintf(stderr, "MISMATCH Ctl: a field beyond ncommit / ninf / error changed\n"); ok = false; }
    if (!ok) fprintf(stderr, "  (after launch %u)\n", launch);
    return ok;
}

static int drive(WfCase& c, const char* label, bool skip_beyond) {
    const Problem& p = c.p;
    State k = start_state(c), m = start_state(c), t = start_state(c);
    std::vector<u32> ps(p.N + 8, POISON), cap(p.N + 8, POISON), ent(p.N + 8, POISON);
    std::vector<u64> sc = p.sc;
    std::vector<RTask> rt = p.rt;
    std::vector<u32> list_off = p.list_off;
    Reach rc, unused;
    std::vector<char> made_before(p.list_node.size(), 0), never(p.list_node.size(), 0);
    u64 differs = 0;
    u32 launch = 0;
    for (const Run& run : c.runs) {
        const u32 ncommit_before = m.ctl.ncommit, ninf_before = m.ctl.ninf;
        model_run(c, m, run, rc, skip_beyond, made_before);
        if (skip_beyond) {   // ... and the TRUE ranking next to it: how far the kernel's rule is from the reference
            model_run(c, t, run, unused, false, never);
            for (u32 i = 0; i < run.count; ++i) differs += t.out[run.j0 + i] != m.out[run.j0 + i];
        }
        for (u32 q = ninf_before; q < m.ctl.ninf; ++q)   // the model's own invariant: the tail sits at the final commit position
            if (m.inf_pos[q] != m.ctl.ncommit || m.ctl.ncommit - ncommit_before + (m.ctl.ninf - ninf_before) != run.count) { fprintf(stderr, "MODEL: a failed task in front of a placed one\n"); return 1; }
        WaterArgs a{};
        a.n_nodes = p.N;
        a.n_words = p.Wn;
        a.xs = c.xs;
        a.j0 = run.j0;
        a.count = run.count;
        a.rt = rt.data();
        a.sc = sc.data();
        a.cpu = k.cpu.data();
        a.mem = k.mem.data();
        a.total = k.total.data();
        a.X = k.X.data();
        a.list_node = k.list_node.data();
        a.list_svc = k.list_svc.data();
        a.list_fail = k.list_fail.data();
        a.list_off = list_off.data();
        a.out_node = k.out.data();
        a.log_node = k.log_node.data();
        a.log_task = k.log_task.data();
        a.log_prev = k.log_prev.data();
        a.last = k.last.data();
        a.inf_task = k.inf_task.data();
        a.inf_pos = k.inf_pos.data();
        a.ctl = &k.ctl;
        a.ps = ps.data();
        a.cap = cap.data();
        a.ent = ent.data();
        emu::launch(WF_THREADS, 0, [a]() { k_waterfill(a); });
        for (u32 q = 0; q < 8; ++q)
            if (ps[p.N + q] != POISON || cap[p.N + q] != POISON || ent[p.N + q] != POISON) { fprintf(stderr, "MISMATCH scratch written beyond n_nodes (launch %u)\n", launch); return 1; }
        if (sc != p.sc || memcmp(rt.data(), p.rt.data(), rt.size() * sizeof(RTask)) != 0 || list_off != p.list_off) { fprintf(stderr, "MISMATCH an input table changed (launch %u)\n", launch); return 1; }
        if (!equal_states(k, m, launch)) {
            print_reach(rc, differs);
            fprintf(stderr, "%s: launch %u (service %u, tasks [%u, %u)) -> FAIL\n", label, launch, p.rt[run.j0].svc, run.j0, run.j0 + run.count);
            return 1;
        }
        for (u32 e = 0; e < m.list_node.size(); ++e)
            if (m.list_node[e] != LIST_EMPTY && p.list_node[e] == LIST_EMPTY) made_before[e] = 1;
        ++launch;
    }
    print_reach(rc, differs);
    fprintf(stderr, "%s: %u nodes, %u tasks in %u launches, %u placed, %u without a node -> OK\n", label, p.N, p.T, launch, m.ctl.ncommit - c.ncommit0, m.ctl.ninf - c.ninf0);
    return 0;
}

// ---- problems ---------------------------------------------------------------------------------------------------------------------
struct SvcSpec {
    u32 sc = 0, flags = 0;
    i64 cpu = 0, mem = 0;
    u64 maxrep = 0;
    std::vector<std::array<u32, 3>> entries;   // (node or LIST_EMPTY, svcCount, failures), in list order
};

// the tables of a case from its services, node rows and the order of the runs (a run: service, length)
static void assemble(WfCase& c, const std::vector<SvcSpec>& sv, const std::vector<std::pair<u32, u32>>& order) {
    Problem& p = c.p;
    p.S = (u32)sv.size();
    p.Wn = (p.N + 63) / 64;
    c.xs = p.Wn + 1;
    std::vector<u32> ntasks(p.S, 0);
    p.T = 0;
    for (const auto& o : order) { ntasks[o.first] += o.second; p.T += o.second; }
    p.X.assign((size_t)p.S * c.xs, 0);
    for (u32 s = 0; s < p.S; ++s) p.X[(size_t)s * c.xs + p.Wn] = POISON64;   // the word between two rows belongs to nobody
    p.list_off.assign(p.S + 1, 0);
    std::vector<u32> first_free(p.S, 0);
    for (u32 s = 0; s < p.S; ++s) {
        p.list_off[s] = (u32)p.list_node.size();
        for (const auto& e : sv[s].entries) {
            p.list_node.push_back(e[0]);
            p.list_svc.push_back(e[1]);
            p.list_fail.push_back(e[2]);
            if (e[0] != LIST_EMPTY) p.X[(size_t)s * c.xs + (e[0] >> 6)] |= 1ull << (e[0] & 63);
        }
        first_free[s] = (u32)p.list_node.size();
        for (u32 i = 0; i < ntasks[s]; ++i) {   // one reserved slot per task; the kernel writes all three words when it takes one
            p.list_node.push_back(LIST_EMPTY);
            p.list_svc.push_back(POISON);
            p.list_fail.push_back(POISON);
        }
    }
    p.list_off[p.S] = (u32)p.list_node.size();
    p.rt.resize(p.T);
    std::vector<u32> rank(p.S, 0);
    u32 j = 0;
    for (const auto& o : order) {
        c.runs.push_back({j, o.second});
        for (u32 i = 0; i < o.second; ++i, ++j) {
            RTask& r = p.rt[j];
            memset(&r, 0, sizeof r);
            const SvcSpec& v = sv[o.first];
            r.svc = o.first;
            r.sc = v.sc;
            r.flags = v.flags;
            r.cpu = v.cpu;
            r.mem = v.mem;
            r.maxrep = v.maxrep;
            r.slot = first_free[o.first] + rank[o.first]++;
        }
    }
    if (c.last0.empty()) c.last0.assign(p.N, -1);
}

static int seeded(u32 seed, u32 N, u32 len) {
    std::mt19937_64 g(0x9E3779B97F4A7C15ull * (seed + 1) + 0x77A7);
    auto rnd = [&](u32 k) { return (u32)(g() % k); };
    WfCase c;
    Problem& p = c.p;
    p.N = N;
    const u32 Wn = (N + 63) / 64;
    const i64 UC = 1000, UM = 1ll << 20;
    p.cpu.resize(N);
    p.mem.resize(N);
    p.total.resize(N);
    const u32 tmode = rnd(3);   // 0: every node at the same count (ties by index alone); 1: a few counts; 2: more of them
    for (u32 n = 0; n < N; ++n) {
        p.cpu[n] = (i64)rnd(7) * UC + (rnd(4) ? 0 : rnd((u32)UC));   // k x the unit, now and then a remainder
        p.mem[n] = (i64)rnd(7) * UM + (rnd(4) ? 0 : rnd((u32)UM));
        if (rnd(25) == 0) (rnd(2) ? p.cpu[n] : p.mem[n]) = -(i64)(1 + rnd(500));   // over-committed
        if (len != 3 && rnd(40) == 0) { p.cpu[n] = (1ll << 62) + rnd(5); p.mem[n] = (1ll << 62) - rnd(5); }
        p.total[n] = tmode == 0 ? 4 : tmode == 1 ? rnd(3) : rnd(7);
    }
    // static classes: 0 nearly all nodes, 1 about half, 2 none, 3 all
    p.n_sc = 4;
    p.sc.assign((size_t)p.n_sc * Wn, 0);
    for (u32 n = 0; n < N; ++n) {
        if (rnd(30)) p.sc[0 * Wn + (n >> 6)] |= 1ull << (n & 63);
        if (rnd(2)) p.sc[1 * Wn + (n >> 6)] |= 1ull << (n & 63);
        p.sc[3 * (size_t)Wn + (n >> 6)] |= 1ull << (n & 63);
    }
    std::vector<SvcSpec> sv(3);
    for (u32 s = 0; s < 3; ++s) {
        SvcSpec& v = sv[s];
        v.sc = s == 2 ? (rnd(3) ? rnd(4) : 2u) : (rnd(4) ? rnd(2) : 3u);
        const u32 kind = len == 3 && s == 0 ? 3 : rnd(5);   // 0: no reservations, 1: cpu, 2: memory, 3: both, 4: the filter on with 0 / 0
        if (kind) v.flags |= RT_RES;
        if (kind == 1 || kind == 3) v.cpu = UC * (1 + rnd(2));
        if (kind == 2 || kind == 3) v.mem = UM * (1 + rnd(2));
        if (rnd(3) == 0) { v.flags |= RT_MAXREP; v.maxrep = 1u << rnd(3); }
        std::vector<u32> nodes;
        for (u32 n = 0; n < N; ++n)
            if (rnd(3) == 0) nodes.push_back(n);
        std::shuffle(nodes.begin(), nodes.end(), g);
        for (u32 n : nodes) {
            if (rnd(8) == 0) v.entries.push_back({LIST_EMPTY, 7u, 9u});   // a hole: whatever its other words say
            u32 cnt = rnd(5), fl = 0;
            switch (rnd(6)) {
            case 2: fl = 1 + rnd(MAX_FAILURES - 1); break;
            case 3: fl = MAX_FAILURES; break;
            case 4: fl = MAX_FAILURES + 1 + rnd(4); break;
            default: break;
            }
            if (!cnt && !fl) cnt = 1;
            v.entries.push_back({n, cnt, fl});
        }
        if (rnd(2)) v.entries.push_back({LIST_EMPTY, 0u, 0u});
    }
    auto eligible = [&](u32 s) {
        u32 k = 0;
        for (u32 w = 0; w < Wn; ++w) k += (u32)__builtin_popcountll(p.sc[(size_t)sv[s].sc * Wn + w]);
        return std::max(k, 1u);
    };
    const u32 EA = eligible(0), EB = eligible(1), EC = eligible(2);
    std::vector<std::pair<u32, u32>> order;
    switch (len) {
    case 0: order = {{0, 1}, {1, 2}, {0, 2}, {2, 1}, {1, 1}}; break;
    case 1: order = {{0, EA}, {1, EB + 1}, {0, std::max(EA / 2, 1u)}, {2, EC}, {1, 2}}; break;
    case 2: order = {{0, 3 * EA + 5}, {1, 2}, {0, 2 * EA + 1}, {2, 2 * EC + 3}, {1, 3 * EB}}; break;
    default: order = {{0, 7 * EA + 9}, {1, EB}, {0, 3}, {2, EC + 1}, {1, 1}}; break;   // 7 laps of a cluster whose nodes hold at most 6 units each
    }
    assemble(c, sv, order);
    if (rnd(3)) {   // the batch's earlier stretches left commits, chains and tasks without a node behind
        c.ncommit0 = 3 + rnd(20);
        c.ninf0 = rnd(2) ? 0 : 1 + rnd(9);
        for (u32 n = 0; n < N; ++n)
            if (rnd(4) == 0) c.last0[n] = (int32_t)rnd(c.ncommit0);
    }
    char label[96];
    snprintf(label, sizeof label, "seeded seed %u N %u len %u", seed, N, len);
    return drive(c, label, false);
}

// a small cluster by hand: every node eligible (class 0), `N` nodes at task count 0 with roomy residuals, one service per spec
static WfCase plain(u32 N) {
    WfCase c;
    Problem& p = c.p;
    p.N = N;
    p.n_sc = 2;
    p.sc.assign((size_t)2 * ((N + 63) / 64), 0);
    for (u32 n = 0; n < N; ++n) p.sc[n >> 6] |= 1ull << (n & 63);   // row 1 stays empty
    p.cpu.assign(N, 1'000'000);
    p.mem.assign(N, 1'000'000);
    p.total.assign(N, 0);
    return c;
}
static void ineligible(WfCase& c, u32 n) { c.p.sc[n >> 6] &= ~(1ull << (n & 63)); }

static int edge(const std::string& name) {
    const u32 F0 = MAX_FAILURES - 1;   // failures = class + F0 for a class above 0
    if (name == "error") {   // Ctl.error already set: the launch writes nothing at all
        WfCase c = plain(70);
        c.error0 = ERR_LEVEL_RANGE;
        c.ncommit0 = 4;
        c.ninf0 = 2;
        std::vector<SvcSpec> sv(1);
        sv[0].entries = {{3u, 1u, 0u}};
        assemble(c, sv, {{0, 9}, {0, 1}});
        return drive(c, "edge error", false);
    }
    if (name == "packed_below") {   // the last values the packed key holds: svcCount 2^24 - 1, failure class 254 — ranked by their true values
        WfCase c = plain(4);
        ineligible(c, 2);
        std::vector<SvcSpec> sv(2);
        sv[0].flags = RT_MAXREP;
        sv[0].maxrep = 1ull << 24;   // node 0 takes ONE task (its count must not carry into the class field)
        sv[0].entries = {{0u, (1u << 24) - 1, 0u}, {1u, 3u, 254 + F0}, {3u, (1u << 24) - 1, 254 + F0}};
        sv[1].flags = RT_MAXREP;
        sv[1].maxrep = 1ull << 24;
        sv[1].entries = {{3u, (1u << 24) - 1, 254 + F0}, {LIST_EMPTY, 0u, 0u}, {1u, (1u << 24) - 1, 254 + F0}, {0u, (1u << 24) - 1, 254 + F0}};
        assemble(c, sv, {{0, 4}, {1, 5}});
        return drive(c, "edge packed_below", false);
    }
    if (name == "packed_at") {   // the first values beyond it: svcCount 2^24, failure class 255. The reference ranks such a node last; the
                                 // kernel gives it capacity 0 for the whole run. Compared with the model under THAT rule; the distance to
                                 // the true ranking is printed (true_model_differs) and asserted by the test.
        WfCase c = plain(4);
        ineligible(c, 3);
        c.p.cpu = {1000, 1'000'000, 2000, 1'000'000};
        std::vector<SvcSpec> sv(1);
        sv[0].flags = RT_RES;
        sv[0].cpu = 1000;
        sv[0].entries = {{0u, 1u << 24, 0u}, {1u, 0u, 255 + F0}};
        assemble(c, sv, {{0, 5}});
        return drive(c, "edge packed_at", true);
    }
    if (name == "clamp") {   // residuals near 2^62 against a reservation of 1: the quotient is far beyond 32 bits
        WfCase c = plain(3);
        c.p.cpu = {(1ll << 62) + 5, 1ll << 62, 3};
        c.p.mem = {1ll << 62, (1ll << 62) + 1, 1ll << 62};
        std::vector<SvcSpec> sv(1);
        sv[0].flags = RT_RES;
        sv[0].cpu = 1;
        sv[0].mem = 1;
        assemble(c, sv, {{0, 300}});
        return drive(c, "edge clamp", false);
    }
    if (name == "negzero") {   // the filter on with a reservation of 0 / 0: a negative residual still fails it; a residual of 0 does not
        WfCase c = plain(5);
        c.p.cpu = {-5, 10, 0, 10, 0};
        c.p.mem = {10, -1, 0, 10, 10};
        std::vector<SvcSpec> sv(2);
        sv[0].flags = RT_RES;
        sv[1].flags = 0;   // the same cluster without the filter: every node is used
        assemble(c, sv, {{0, 7}, {1, 7}});
        return drive(c, "edge negzero", false);
    }
    if (name == "exactk") {   // residuals of exactly k x the reservation, one below and one above it; cpu only, memory only, both
        WfCase c = plain(6);
        c.p.cpu = {3000, 2999, 3001, 1'000'000, 1'000'000, 2000};
        c.p.mem = {1'000'000, 1'000'000, 1'000'000, 400, 399, 600};
        std::vector<SvcSpec> sv(3);
        sv[0].flags = RT_RES;
        sv[0].cpu = 1000;
        sv[1].flags = RT_RES;
        sv[1].mem = 200;
        sv[2].flags = RT_RES;
        sv[2].cpu = 500;
        sv[2].mem = 100;
        assemble(c, sv, {{0, 3}, {1, 2}, {2, 40}, {0, 2}});
        return drive(c, "edge exactk", false);
    }
    fprintf(stderr, "unknown edge %s\n", name.c_str());
    return 2;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "seeded" && argc >= 5) return seeded((u32)atoi(argv[2]), (u32)atoi(argv[3]), (u32)atoi(argv[4]));
    if (mode == "edge" && argc >= 3) return edge(argv[2]);
    fprintf(stderr, "usage: %s seeded seed N len(0..3) | edge error|packed_below|packed_at|clamp|negzero|exactk\n", argv[0]);
    return 2;
}
