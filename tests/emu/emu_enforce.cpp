// emu_enforce.cpp — runs k_enforce_generic (swarmkit_amd/csrc/swp_enforce.hpp: the enforcer sweep for nodes whose tasks hold
// AssignedGenericResources, one wave per node) on CPU fibers (wv_emu.hpp) against a sequential model written from the reference's
// three functions: the loop body of rejectNoncompliantTasks (constraint_enforcer.go:114-202), HasResource (validate.go:54-85) and
// ConsumeNodeResources + remove (helpers.go:58-111). The model keeps a node's list as a vector it erases from — no "gone" flags, no
// chunks, no lanes. TEST INFRASTRUCTURE (tests/test_emu_enforce.py).
//
//   emu_enforce sweep <seed> <nodes>
// Every node goes through the kernel, the ones without any assignment too (the path k_enforce takes with the same enf_step). Compared:
// every verdict byte (the array starts as 0xAA: a byte nobody wrote shows), and for the lists longer than a wave what is left of them.
// Prints a "reach sweep: ..." line — what the MODEL's run came across — then "-> OK" or the first difference.
#include "wv_emu.hpp"

#define SWP_ENF_KERNELS
#include "../../swarmkit_amd/csrc/swp_enforce.hpp"

#include <string>

using namespace swpdev;

struct Rng {
    u64 s;
    explicit Rng(u64 seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x1234567ull) {}
    u64 next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return s * 0x2545F4914F6CDD1Dull; }
    u32 below(u32 n) { return (u32)(next() % n); }
    bool chance(u32 pct) { return below(100) < pct; }
};

// ---- the model ----
struct MRes { u32 kind; bool named; i64 value; };
struct Reach {
    u64 brk = 0, behind_break_rejected = 0, type_mismatch = 0, kind_twice = 0, two_assignments = 0, exact_zero = 0, long_list = 0, decided_past_64 = 0,
        claimed = 0, plain_rejected = 0, skipped = 0, nil_or_empty = 0;
};

static bool m_has_resource(const MRes& res, const std::vector<MRes>& resources, Reach& rc, size_t* decided_at) {
    for (size_t i = 0; i < resources.size(); ++i) {
        const MRes& r = resources[i];
        if (res.kind != r.kind) continue;
        *decided_at = i;
        if (!r.named) {
            if (res.named) { rc.type_mismatch++; return false; }
            if (res.value > r.value) return false;
            return true;
        }
        if (!res.named) { rc.type_mismatch++; return false; }
        if (res.value != r.value) continue;
        return true;
    }
    *decided_at = resources.size();
    return false;
}
static bool m_remove(MRes& na, const MRes& r, Reach& rc) {
    if (!r.named) {
        if (na.named) { rc.type_mismatch++; return false; }
        na.value = (i64)((u64)na.value - (u64)r.value);
        if (na.value == 0) rc.exact_zero++;
        return na.value <= 0;
    }
    if (!na.named) { rc.type_mismatch++; return false; }
    return r.value == na.value;
}
static void m_consume(std::vector<MRes>& avail, const std::vector<MRes>& res, Reach& rc) {
    std::vector<MRes> kept;
    std::vector<u32> discrete_hits(res.size(), 0);
    for (MRes na : avail) {
        bool gone = false;
        u32 subtracted = 0;
        for (size_t q = 0; q < res.size() && !gone; ++q) {
            if (na.kind != res[q].kind) continue;
            if (!res[q].named && !na.named) { subtracted++; discrete_hits[q]++; }
            if (m_remove(na, res[q], rc)) gone = true;
        }
        if (subtracted >= 2) rc.two_assignments++;
        if (!gone) kept.push_back(na);
    }
    for (u32 h : discrete_hits)
        if (h >= 2) rc.kind_twice++;   // one assignment entry met two Discrete entries of its kind
    avail.swap(kept);
}

struct Problem {
    u32 n_words = 0, n_cls = 0;
    std::vector<u64> con;
    std::vector<EnfNode> nodes;
    std::vector<EnfTask> tasks;
    std::vector<u32> noff{0u}, toff{0u};
    std::vector<EnfRes> nres, tres;
};

static EnfRes pack(const MRes& m) { return EnfRes{m.kind, m.named ? ENF_NAMED : 0u, m.value}; }

static Problem generate(u64 seed, u32 n_nodes) {
    Rng g(seed);
    Problem p;
    const u32 slots = n_nodes * 2 + 70;
    p.n_words = (slots + 63) / 64;
    p.n_cls = 5;
    p.con.assign((size_t)p.n_cls * p.n_words, 0);
    for (u64& wd : p.con) wd = g.next() | g.next();   // three nodes in four match a class
    static const i64 big[] = {0, -3, 1ll << 31, (1ll << 31) + 5, 1ll << 40, 3000000000ll};
    for (u32 i = 0; i < n_nodes; ++i) {
        // the node's list: a few kinds; a kind may come twice, Discrete and Named mixed; one node in six has a list longer than a wave
        std::vector<MRes> list;
        const bool longl = g.chance(17);
        const u32 len = longl ? 65 + g.below(140) : g.below(4) == 0 ? 0 : 1 + g.below(9);
        for (u32 k = 0; k < len; ++k) {
            MRes m;
            m.kind = 1 + g.below(longl ? 2 : 4);
            m.named = longl ? !g.chance(4) : g.chance(50);
            m.value = m.named ? (i64)g.below(longl ? 120 : 6) : g.chance(8) ? big[g.below(6)] : (i64)g.below(6);
            list.push_back(m);
        }
        for (const MRes& m : list) p.nres.push_back(pack(m));
        p.noff.push_back((u32)p.nres.size());
        EnfNode nd{};
        nd.node = g.below(slots);
        nd.first = (u32)p.tasks.size();
        nd.count = g.below(14);
        nd.cpu = (i64)g.below(9) * 1000;
        nd.mem = (i64)g.below(9) * 1000;
        const bool generic_node = !g.chance(25);
        for (u32 k = 0; k < nd.count; ++k) {
            EnfTask t{};
            static const u32 states[] = {0, 64, 192, 384, 512, 512, 512, 512, 576, 640, 704};
            t.desired = g.chance(80) ? 512u : states[g.below(11)];
            t.state = g.chance(80) ? 512u : states[g.below(11)];
            t.cls_con = g.chance(40) ? 1 + g.below(p.n_cls - 1) : 0u;
            if (g.chance(50)) {
                t.flags = 1;
                t.cpu = (i64)g.below(4) * 500;
                t.mem = (i64)g.below(4) * 500;
            }
            p.tasks.push_back(t);
            if (generic_node && g.chance(55)) {
                const u32 na = g.below(4);   // (0: an empty list, which behaves like nil)
                for (u32 q = 0; q < na; ++q) {
                    MRes m;
                    if (!list.empty() && g.chance(75)) {   // something the node lists: a name as it stands, a Discrete value up to what is there
                        m = list[g.below((u32)list.size())];
                        if (!m.named && m.value > 0 && m.value < 100) m.value = 1 + (i64)g.below((u32)m.value);
                        if (g.chance(6)) m.named = !m.named;
                    } else {
                        m.kind = 1 + g.below(4);
                        m.named = g.chance(50);
                        m.value = m.named ? (i64)g.below(120) : g.chance(10) ? big[g.below(6)] : (i64)g.below(4);
                    }
                    if (q > 0 && g.chance(35)) {   // a second assignment of the same kind
                        const EnfRes& prev = p.tres.back();
                        m.kind = prev.kind;
                        m.named = (prev.flags & ENF_NAMED) != 0;
                        m.value = m.named ? (i64)g.below(6) : 1;
                    }
                    p.tres.push_back(pack(m));
                }
            }
            p.toff.push_back((u32)p.tres.size());
        }
        p.nodes.push_back(nd);
    }
    return p;
}

static int sweep(u64 seed, u32 n_nodes) {
    Problem p = generate(seed, n_nodes);
    const u32 T = (u32)p.tasks.size();
    // ---- the model: one node after the other ----
    Reach rc;
    std::vector<unsigned char> want(T, 0);
    std::vector<std::vector<MRes>> left(n_nodes);
    for (u32 i = 0; i < n_nodes; ++i) {
        const EnfNode& nd = p.nodes[i];
        std::vector<MRes> avail;
        for (u32 q = p.noff[i]; q < p.noff[i + 1]; ++q) avail.push_back(MRes{p.nres[q].kind, (p.nres[q].flags & ENF_NAMED) != 0, p.nres[q].value});
        i64 cpu = nd.cpu, mem = nd.mem;
        bool broke = false;
        for (u32 t = nd.first; t < nd.first + nd.count; ++t) {
            const EnfTask& tk = p.tasks[t];
            const bool skip = tk.desired < 192u || tk.desired > 576u || tk.state >= 576u;
            const bool con_fails = tk.cls_con && !((p.con[(size_t)tk.cls_con * p.n_words + (nd.node >> 6)] >> (nd.node & 63)) & 1ull);
            const bool res_fails = !con_fails && (tk.flags & 1u) && (tk.mem > mem || tk.cpu > cpu);
            if (broke) {   // (what the walk would have said: the reach counter only)
                if (!skip && (con_fails || res_fails)) rc.behind_break_rejected++;
                continue;
            }
            if (skip) { rc.skipped++; continue; }
            if (con_fails || res_fails) { want[t] = 1; rc.plain_rejected++; continue; }
            if (tk.flags & 1u) { mem -= tk.mem; cpu -= tk.cpu; }
            if (p.toff[t + 1] == p.toff[t]) { rc.nil_or_empty++; continue; }
            std::vector<MRes> assigned;
            for (u32 q = p.toff[t]; q < p.toff[t + 1]; ++q) assigned.push_back(MRes{p.tres[q].kind, (p.tres[q].flags & ENF_NAMED) != 0, p.tres[q].value});
            if (avail.size() > 64) rc.long_list++;
            bool there = true;
            for (const MRes& ta : assigned) {
                size_t at = 0;
                const bool has = m_has_resource(ta, avail, rc, &at);
                if (at >= 64 && at < avail.size()) rc.decided_past_64++;
                if (!has) { there = false; break; }
            }
            if (!there) { want[t] = 1; broke = true; rc.brk++; continue; }
            m_consume(avail, assigned, rc);
            rc.claimed++;
        }
        left[i] = avail;
    }
    // ---- the kernel: every node a wave, four to a workgroup ----
    std::vector<unsigned char> got(T + 1, 0xAA);
    std::vector<EnfRes> work = p.nres;
    std::vector<u32> src(n_nodes);
    for (u32 i = 0; i < n_nodes; ++i) src[i] = i;
    EnfGenArgs a{};
    a.n_gen = n_nodes;
    a.n_words = p.n_words;
    a.nodes = p.nodes.data();
    a.src = src.data();
    a.tasks = p.tasks.data();
    a.con = p.con.data();
    a.node_res_off = p.noff.data();
    a.node_res = p.nres.data();
    a.work = work.data();
    a.task_res_off = p.toff.data();
    a.task_res = p.tres.data();
    a.out = got.data();
    for (u32 b = 0; b < (n_nodes + 3) / 4; ++b) {
        emu::blockidx() = b;
        emu::launch(256, 0, [&] { k_enforce_generic(a); });
    }
    emu::blockidx() = 0;
    fprintf(stderr,
            "reach sweep: break_loop=%llu behind_break_rejected=%llu type_mismatch=%llu kind_twice=%llu two_assignments=%llu exact_zero=%llu long_list=%llu "
            "decided_past_64=%llu claimed=%llu plain_rejected=%llu skipped=%llu nil_or_empty=%llu\n",
            (unsigned long long)rc.brk, (unsigned long long)rc.behind_break_rejected, (unsigned long long)rc.type_mismatch, (unsigned long long)rc.kind_twice,
            (unsigned long long)rc.two_assignments, (unsigned long long)rc.exact_zero, (unsigned long long)rc.long_list, (unsigned long long)rc.decided_past_64,
            (unsigned long long)rc.claimed, (unsigned long long)rc.plain_rejected, (unsigned long long)rc.skipped, (unsigned long long)rc.nil_or_empty);
    for (u32 i = 0; i < n_nodes; ++i)
        for (u32 t = p.nodes[i].first; t < p.nodes[i].first + p.nodes[i].count; ++t)
            if (got[t] != want[t]) {
                fprintf(stderr, "MISMATCH node %u (list of %u) task %u (its %u.): emu %u model %u\n", i, p.noff[i + 1] - p.noff[i], t, t - p.nodes[i].first, got[t], want[t]);
                return 1;
            }
    if (got[T] != 0xAA) { fprintf(stderr, "MISMATCH a verdict byte behind the last task was written\n"); return 1; }
    for (u32 i = 0; i < n_nodes; ++i) {
        const u32 r0 = p.noff[i], r1 = p.noff[i + 1];
        std::vector<MRes> dev;
        for (u32 q = r0; q < r1; ++q)
            if (r1 - r0 > 64) {
                if (!(work[q].flags & ENF_GONE)) dev.push_back(MRes{work[q].kind, (work[q].flags & ENF_NAMED) != 0, work[q].value});
            } else if (memcmp(&work[q], &p.nres[q], sizeof(EnfRes)) != 0) {
                fprintf(stderr, "MISMATCH node %u: a list that fits the wave was written to the work copy\n", i);
                return 1;
            }
        if (r1 - r0 <= 64) continue;
        bool same = dev.size() == left[i].size();
        for (size_t k = 0; same && k < dev.size(); ++k) same = dev[k].kind == left[i][k].kind && dev[k].named == left[i][k].named && dev[k].value == left[i][k].value;
        if (!same) { fprintf(stderr, "MISMATCH node %u: what is left of its list of %u: emu %zu entries, model %zu\n", i, r1 - r0, dev.size(), left[i].size()); return 1; }
    }
    fprintf(stderr, "sweep seed %llu: %u nodes, %u tasks -> OK\n", (unsigned long long)seed, n_nodes, T);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && std::string(argv[1]) == "sweep") return sweep(strtoull(argv[2], nullptr, 10), (u32)atoi(argv[3]));
    fprintf(stderr, "usage: emu_enforce sweep <seed> <nodes>\n");
    return 2;
}
