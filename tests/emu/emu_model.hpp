// emu_model.hpp — random problems and the plain sequential restatement of the resolvers' semantics, shared by the CPU
// emulation harnesses (emu_resolve6.cpp, emu_resolve7.cpp, emu_scan.cpp). TEST INFRASTRUCTURE; not part of the product.
//
// The model follows k_resolve (swp_device.hpp): plain nodes by (level, index) with a re-check of the dynamic filters, then the
// service's exception list by nodeLess, scheduler.go:708-735; NodeInfo.addTask, nodeinfo.go:108-154.
#pragma once
#include <algorithm>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "../../swarmkit_amd/csrc/swp_volumes.hpp"   // (the records of the device tables only: VolMount, VolDyn, VolView)

using namespace swpdev;

// =============================================================================================================================
// CSI volumes: a per-node, per-mount restatement of VolumeSet (oracle/swk_oracle.cpp: check_volume, is_available_on_node,
// choose_task_volumes, reserve_task_volumes, is_in_topology; volumes.go:101-316, topology.go:23-47, filter.go:424-432), written from
// that text and not from swp_volumes.hpp: usage is kept as the reference keeps it — per volume the map task -> (node, read-only) —
// and what the device holds ({n_tasks, n_writers, pin}) is DERIVED from it for comparison only. Names are ids: plugin, subdomain
// and segment ids as SWP_SPACE_CSI hands them out (segment id 0 = the empty string).
// =============================================================================================================================
enum { MV_SH_NONE = 0, MV_SH_READ_ONLY = 1, MV_SH_ONE_WRITER = 2, MV_SH_ALL = 3 };
struct MVolume {
    bool active = true, multi = false;
    u32 sharing = MV_SH_ALL, driver = 0;
    std::vector<std::vector<std::pair<u32, u32>>> accessible;   // topologies of (subdomain, segment) pairs
};
struct MCsiInfo {
    u32 plugin = 0;
    bool has_topology = false;
    std::vector<std::pair<u32, u32>> segments;   // (subdomain, segment); a subdomain at most once
};
struct MUsage { u32 node; bool ro; };
typedef std::vector<std::map<u64, MUsage>> VolUsage;   // [volume]: task id -> usage (volumeInfo.tasks)

struct VolReach {   // what a MODEL run came across (the conditions a committed case must meet are stated on these)
    u64 check[4][2] = {};   // checkVolume calls by (sharing, read-only mount)
    u64 single_here = 0, single_elsewhere = 0, pin_many = 0;
    u64 fail_first = 0, fail_later = 0, choice_ok = 0, refused_by_own = 0;
};

#define VOL_WRITER_SETS 16
struct VolProblem {
    u32 N = 0;
    std::vector<MVolume> vol;
    std::vector<std::vector<MCsiInfo>> node_csi;   // [N]
    std::vector<std::vector<u32>> group;           // volumes of a group in the order they were created (ascending)
    std::vector<std::vector<VolMount>> set;        // mount sets; set 0 is "no cluster mounts" and stays empty
    VolUsage use0;                                 // usage at start-up
    u32 writer_set = 0;                            // the first of VOL_WRITER_SETS sets: a writing mount of an unused multi-node volume for one writer, no topologies
    u32 easy_set = 0;                              // a set that finds its volume on every node (a read-only mount of a multi-node volume all may share, no topologies)
    mutable VolReach reach;

    // IsInTopology(top(node, driver(vol)), accessible(vol))
    bool in_topology(u32 v, u32 node) const {
        const MCsiInfo* top = nullptr;
        for (const MCsiInfo& c : node_csi[node])
            if (c.plugin == vol[v].driver) { top = &c; break; }   // the first entry of the plugin
        if (!top || !top->has_topology || vol[v].accessible.empty()) return true;
        for (const auto& topology : vol[v].accessible) {
            bool all = true;
            for (const auto& want : topology) {
                u32 have = 0;   // a missing subdomain reads as ""
                for (const auto& s : top->segments)
                    if (s.first == want.first) { have = s.second; break; }
                if (have != want.second) { all = false; break; }
            }
            if (all) return true;
        }
        return false;
    }
    bool check_volume(const VolUsage& use, u32 v, u32 node, bool ro, bool count = true) const {
        const MVolume& m = vol[v];
        if (!m.active) return false;
        if (count) {
            reach.check[m.sharing][ro ? 1 : 0]++;
            bool many = false;
            for (const auto& kv : use[v]) many = many || kv.second.node != use[v].begin()->second.node;
            if (many) reach.pin_many++;
            if (!m.multi && !many && !use[v].empty()) (use[v].begin()->second.node == node ? reach.single_here : reach.single_elsewhere)++;
        }
        if (!m.multi)
            for (const auto& kv : use[v])
                if (kv.second.node != node) return false;
        switch (m.sharing) {
        case MV_SH_NONE:
            if (!use[v].empty()) return false;
            break;
        case MV_SH_ONE_WRITER:
            if (!ro)
                for (const auto& kv : use[v])
                    if (!kv.second.ro) return false;
            break;
        case MV_SH_READ_ONLY:
            if (!ro) return false;
            break;
        default: break;
        }
        return in_topology(v, node);
    }
    u32 available_on_node(const VolUsage& use, const VolMount& m, u32 node, bool count = true) const {
        if (m.ref == VOL_NONE) return VOL_NONE;   // a name (a group) no volume carries
        if (m.is_group) {
            for (u32 v : group[m.ref])
                if (check_volume(use, v, node, m.ro != 0, count)) return v;
            return VOL_NONE;
        }
        return check_volume(use, m.ref, node, m.ro != 0, count) ? m.ref : VOL_NONE;
    }
    bool filter(const VolUsage& use, u32 s, u32 node) const {   // VolumesFilter.Check: ANY mount has a volume
        for (const VolMount& m : set[s])
            if (available_on_node(use, m, node) != VOL_NONE) return true;
        return false;
    }
    // chooseTaskVolumes: out[i] = the volume of mount i (VOL_NONE from the failing one on); returns the attachments (0: a mount failed,
    // *failed = which). `use` is left as it was: the temporary reservations are released again.
    u32 choose(VolUsage& use, u32 s, u32 node, u64 task, u32* out, u32* failed) const {
        for (u32 i = 0; i < VOL_MAX_MOUNTS; ++i) out[i] = VOL_NONE;
        std::vector<std::pair<u32, bool>> had;   // (the task is new in every use of this model: nothing to restore but absence)
        u32 n = 0;
        bool ok = true;
        for (const VolMount& m : set[s]) {
            const u32 v = available_on_node(use, m, node);
            if (n > 0) {   // would the answer be another one without this task's own temporary reservations?
                VolUsage bare = use;
                for (auto& u : bare) u.erase(task);
                if (available_on_node(bare, m, node, false) != v) reach.refused_by_own++;
            }
            if (v == VOL_NONE) {
                if (failed) *failed = n;
                (n == 0 ? reach.fail_first : reach.fail_later)++;
                ok = false;
                break;
            }
            use[v][task] = MUsage{node, m.ro != 0};
            out[n++] = v;
        }
        for (u32 i = 0; i < n; ++i) use[out[i]].erase(task);
        if (ok) reach.choice_ok++;
        return ok ? n : 0;
    }
    // reserveTaskVolumes: every attachment in order, info.tasks[task] overwritten — ro_reserve is the ReadOnly the reference finds for
    // the attachment's (Source, Target)
    void reserve(VolUsage& use, u32 s, u32 node, u64 task, const u32* att, u32 n) const {
        for (u32 i = 0; i < n; ++i) use[att[i]][task] = MUsage{node, set[s][i].ro_reserve != 0};
    }
    // the device's usage numbers, derived. pin: none / the one node / many. `code`: how a node is written on the replica that is asked
    template <class Code> VolDyn derive(const VolUsage& use, u32 v, Code code) const {
        VolDyn d{0, 0, VOL_PIN_NONE, 0};
        std::set<u32> nodes;
        for (const auto& kv : use[v]) {
            d.n_tasks++;
            if (!kv.second.ro) d.n_writers++;
            nodes.insert(kv.second.node);
        }
        if (nodes.size() == 1) d.pin = code(*nodes.begin());
        if (nodes.size() > 1) d.pin = VOL_PIN_MANY;
        return d;
    }
    VolDyn derive(const VolUsage& use, u32 v) const { return derive(use, v, [](u32 n) { return n; }); }
};

// the device tables of a VolProblem (what the engine uploads): T from the model's IsInTopology
struct VolTables {
    u32 Wn = 0;
    std::vector<u32> vflags, grp_off, grp_vol, ms_off;
    std::vector<VolDyn> vdyn;
    std::vector<u64> T;
    std::vector<VolMount> ms_mount;
    VolView view() {
        VolView v{};
        v.n_vol = (u32)vflags.size();
        v.n_words = Wn;
        v.vflags = vflags.data();
        v.vdyn = vdyn.data();
        v.T = T.data();
        v.grp_off = grp_off.data();
        v.grp_vol = grp_vol.data();
        v.ms_off = ms_off.data();
        v.ms_mount = ms_mount.data();
        return v;
    }
};
// nodes [first, first + cnt) re-indexed from 0 (a shard's replica); `code`: a global node as this replica writes it
template <class Code> static VolTables vol_tables(const VolProblem& vp, u32 first, u32 cnt, Code code) {
    VolTables t;
    t.Wn = (cnt + 63) / 64;
    const u32 V = (u32)vp.vol.size();
    t.T.assign((size_t)V * t.Wn, 0);
    for (u32 v = 0; v < V; ++v) {
        const MVolume& m = vp.vol[v];
        t.vflags.push_back((m.active ? VOL_ACTIVE : 0u) | (m.multi ? VOL_MULTI : 0u) | (m.sharing << VOL_SHARING_SHIFT));
        t.vdyn.push_back(vp.derive(vp.use0, v, code));
        for (u32 i = 0; i < cnt; ++i)
            if (vp.in_topology(v, first + i)) t.T[(size_t)v * t.Wn + (i >> 6)] |= 1ull << (i & 63);
    }
    t.grp_off.push_back(0);
    for (const auto& g : vp.group) {
        for (u32 v : g) t.grp_vol.push_back(v);
        t.grp_off.push_back((u32)t.grp_vol.size());
    }
    t.ms_off.push_back(0);
    for (const auto& s : vp.set) {
        for (const VolMount& m : s) t.ms_mount.push_back(m);
        t.ms_off.push_back((u32)t.ms_mount.size());
    }
    t.grp_vol.push_back(0);   // (never empty: .data() of an empty vector may be null)
    t.ms_mount.push_back(VolMount{0, VOL_NONE, 0, 0});
    return t;
}
static VolTables vol_tables(const VolProblem& vp) { return vol_tables(vp, 0, vp.N, [](u32 n) { return n; }); }

// Volumes over every scope x sharing x availability, groups (an empty one, one whose volumes all fail), mount sets of 1 ..
// VOL_MAX_MOUNTS mounts, start-up usage. Its own generator: make_problem's stream is not touched.
// extra: random volumes beyond the systematic ones; n_sets: random mount sets beyond the constructed ones; hot: mount sets that all name
// ONE single-node volume (sets [1, hot]) — many tasks after one pinned volume.
static VolProblem make_volumes(u32 seed, u32 N, u32 extra, u32 n_sets, u32 hot = 0) {
    std::mt19937_64 g(0x9E3779B97F4A7C15ull * (seed + 1) + 0xC51);
    auto rnd = [&](u32 k) { return (u32)(g() % k); };
    VolProblem vp;
    vp.N = N;
    // nodes: 0 .. 3 CSIInfo entries of plugins 1 .. 3 (the same plugin twice now and then: the first counts), some without a topology
    vp.node_csi.resize(N);
    for (u32 n = 0; n < N; ++n) {
        const u32 k = rnd(6) == 0 ? 0 : 1 + rnd(3);
        for (u32 i = 0; i < k; ++i) {
            MCsiInfo c;
            c.plugin = 1 + rnd(3);
            c.has_topology = rnd(5) != 0;
            for (u32 sd = 1; sd <= 3; ++sd)
                if (rnd(3)) c.segments.push_back({sd, rnd(4)});   // segment 0: the empty string, as good as a missing subdomain
            if (rnd(2)) std::reverse(c.segments.begin(), c.segments.end());
            vp.node_csi[n].push_back(c);
        }
    }
    auto topologies = [&](MVolume& m) {
        const u32 k = rnd(3) == 0 ? 0 : 1 + rnd(3);
        for (u32 i = 0; i < k; ++i) {
            std::vector<std::pair<u32, u32>> t;
            const u32 pairs = rnd(8) == 0 ? 0 : 1 + rnd(2);   // (a topology without segments fits every node that has one)
            for (u32 q = 0; q < pairs; ++q) t.push_back({1 + rnd(3), rnd(12) == 0 ? 0u : 1 + rnd(3)});
            m.accessible.push_back(t);
        }
    };
    for (u32 i = 0; i < 16 + extra; ++i) {
        MVolume m;
        m.multi = i < 16 ? (i & 1) != 0 : rnd(2) != 0;
        m.sharing = i < 16 ? (i >> 1) & 3 : rnd(4);
        m.active = i < 16 ? (i >> 3) == 0 : rnd(8) != 0;
        m.driver = 1 + rnd(3);
        if (rnd(2)) topologies(m);
        vp.vol.push_back(m);
    }
    // single-node volumes in use: one pinned to node 0, one to a node of the LAST node word; one with usages on two nodes; a
    // multi-node volume with pin "many"; no topologies, so that the pin decides
    const u32 V0 = (u32)vp.vol.size();
    for (u32 i = 0; i < 4; ++i) {
        MVolume m;
        m.multi = i == 3;
        m.sharing = i == 1 ? MV_SH_ONE_WRITER : MV_SH_ALL;
        m.driver = 1;
        vp.vol.push_back(m);
    }
    for (u32 i = 0; i < VOL_WRITER_SETS; ++i) {   // ... and multi-node volumes for one writer, unused: the first task that mounts one for writing keeps every later one out, on any node
        MVolume m;
        m.multi = true;
        m.sharing = MV_SH_ONE_WRITER;
        m.driver = 1;
        vp.vol.push_back(m);
    }
    vp.use0.resize(vp.vol.size());
    u64 task = 1ull << 40;   // start-up tasks: ids no batch task has
    vp.use0[V0][task++] = MUsage{0, true};
    vp.use0[V0][task++] = MUsage{0, false};
    vp.use0[V0 + 1][task++] = MUsage{N - 1, true};
    vp.use0[V0 + 2][task++] = MUsage{N / 2, true};
    vp.use0[V0 + 2][task++] = MUsage{N - 1, true};
    vp.use0[V0 + 3][task++] = MUsage{0, false};
    vp.use0[V0 + 3][task++] = MUsage{N - 1, true};
    for (u32 v = 0; v < V0; ++v) {   // readers and writers on a third of the others
        if (rnd(3)) continue;
        const u32 k = 1 + rnd(3), home = rnd(N);
        for (u32 i = 0; i < k; ++i) vp.use0[v][task++] = MUsage{vp.vol[v].multi && rnd(2) ? rnd(N) : home, rnd(2) != 0};
    }
    const u32 V = (u32)vp.vol.size();
    // groups: 0 empty, 1: inactive volumes only, then random ascending subsets
    vp.group.push_back({});
    vp.group.push_back({8, 9, 12, 15});
    vp.group.push_back({0, 1});         // two volumes nobody may share: the second mount of a task takes the next one
    for (u32 i = 0; i < 5; ++i) {
        std::set<u32> s;
        const u32 k = 1 + rnd(4);
        for (u32 q = 0; q < k; ++q) s.insert(rnd(V));
        vp.group.push_back(std::vector<u32>(s.begin(), s.end()));
    }
    const u32 Gn = (u32)vp.group.size();
    auto mount = [&](u32 is_group, u32 ref, u32 ro, u32 ro_reserve) { return VolMount{is_group, ref, ro, ro_reserve}; };
    vp.set.push_back({});   // set 0: no cluster mounts
    for (u32 i = 0; i < hot; ++i) vp.set.push_back({mount(0, V0 + 1, i & 1, i & 1)});
    // constructed sets: the same volume for two mounts (reader then writer, writer then reader: the LAST one speaks); a volume that
    // cannot be shared named twice (the second mount is refused by the task's own reservation); a group of two such volumes named three
    // times (a prefix of two, then the failure); one writer wanted twice; a name no volume carries first, and last; the empty group;
    // the group that always fails behind a mount that is served; eight mounts
    vp.set.push_back({mount(0, 6, 1, 1), mount(0, 6, 0, 0)});
    vp.set.push_back({mount(0, 7, 0, 0), mount(0, 7, 1, 1)});
    vp.set.push_back({mount(0, 1, 0, 0), mount(0, 1, 1, 1)});
    vp.set.push_back({mount(1, 2, 0, 0), mount(1, 2, 0, 0), mount(1, 2, 1, 1)});
    vp.set.push_back({mount(0, 5, 0, 0), mount(0, 5, 0, 0)});
    vp.set.push_back({mount(0, 5, 0, 1), mount(0, 5, 1, 0)});   // ro != ro_reserve
    vp.set.push_back({mount(0, VOL_NONE, 0, 0), mount(0, 7, 0, 0)});
    vp.set.push_back({mount(0, 7, 0, 0), mount(0, VOL_NONE, 0, 0)});
    vp.set.push_back({mount(1, 0, 0, 0)});
    vp.set.push_back({mount(0, 7, 1, 1), mount(1, 1, 0, 0)});
    vp.set.push_back({mount(0, V0, 1, 1)});
    vp.set.push_back({mount(0, V0 + 1, 0, 0), mount(0, V0 + 3, 0, 0)});
    vp.set.push_back({mount(0, V0 + 2, 1, 1)});
    {
        std::vector<VolMount> s;
        for (u32 i = 0; i < VOL_MAX_MOUNTS; ++i) s.push_back(mount(i & 1, (i & 1) ? 2 + rnd(Gn - 2) : (i < 4 ? 7u : 6u), i >= 6, i >= 6));
        vp.set.push_back(s);
    }
    vp.easy_set = (u32)vp.set.size();
    vp.set.push_back({mount(0, V0 + 3, 1, 1)});
    vp.writer_set = (u32)vp.set.size();
    for (u32 i = 0; i < VOL_WRITER_SETS; ++i) vp.set.push_back({mount(0, V0 + 4 + i, 0, 0)});
    for (u32 i = 0; i < n_sets; ++i) {
        std::vector<VolMount> s;
        const u32 k = rnd(3) ? 1 + rnd(2) : 1 + rnd(VOL_MAX_MOUNTS);
        for (u32 q = 0; q < k; ++q) {
            const u32 is_group = rnd(3) == 0, ro = rnd(3) == 0;
            u32 ref = is_group ? rnd(Gn) : rnd(V);
            if (rnd(14) == 0) ref = VOL_NONE;
            if (q > 0 && rnd(5) == 0) { s.push_back(mount(s[q - 1].is_group, s[q - 1].ref, ro, ro)); continue; }   // the mount in front of it again
            s.push_back(mount(is_group, ref, ro, rnd(6) == 0 ? !ro : ro));
        }
        vp.set.push_back(s);
    }
    return vp;
}

// the tasks of a batch that have cluster mounts (feature level 4 of the resolver harnesses) and what the model's run makes of them
struct MountRun {
    const VolProblem* vp = nullptr;
    VolUsage use;                     // the volumes' usage as the model's run goes
    std::vector<u32> csi_of, csi_set; // R6Args.csi_of / csi_set
    std::vector<u32> att;             // [mount tasks][VOL_MAX_MOUNTS]
    u64 with_att = 0, failed_choice = 0, no_node = 0;
    bool is(u32 j) const { return csi_of[j] != 0xFFFFFFFFu; }
    bool passes(u32 j, u32 n) const { return !is(j) || vp->filter(use, csi_set[csi_of[j]], n); }   // VolumesFilter as the volumes stand NOW
    void placed(u32 j, u32 n) {   // chooseTaskVolumes + reserveTaskVolumes (scheduler.go:857-874); a failed choice: assigned without attachments
        if (!is(j)) return;
        const u32 ck = csi_of[j], s = csi_set[ck];
        u32* row = &att[(size_t)ck * VOL_MAX_MOUNTS];
        const u32 n_att = vp->choose(use, s, n, j, row, nullptr);   // (on a failure the row keeps the prefix, as vol_choose documents for the host layer)
        if (n_att) vp->reserve(use, s, n, j, row, n_att);
        (n_att ? with_att : failed_choice)++;
    }
};

// every `every`-th task or so gets a mount set (its own generator: make_problem's stream is not touched); adjacent: tasks 0 and 1 both
// do — two of them at a block's start; last: the batch's last task does; writer: half of them want to WRITE to a
// multi-node volume for one writer, two tasks in a row to the same one (the first one placed keeps the second out, wherever it looks); hot > 0: half of them want the single-node volume that start-up usage pins to the LAST node
// (make_volumes' sets [1, hot])
static MountRun make_mounts(const VolProblem& vp, u32 seed, u32 T, u32 every, bool adjacent, u32 hot, bool last = false, bool writer = false) {
    std::mt19937_64 g(0xD1B54A32D192ED03ull * (seed + 1) + 0x4D);
    auto rnd = [&](u32 k) { return (u32)(g() % k); };
    MountRun m;
    m.vp = &vp;
    m.use = vp.use0;
    m.csi_of.assign(T, 0xFFFFFFFFu);
    u32 n_writers = 0;
    for (u32 j = 0; j < T; ++j) {
        const bool on = rnd(every) == 0, h = rnd(2) == 0;
        const u32 any = 1 + rnd((u32)vp.set.size() - 1), pinned = 1 + rnd(std::max(hot, 1u));
        const bool end = last && j + 1 == T;   // the batch's last task: a mount task that any node serves
        if (!on && !(adjacent && j < 2) && !end) continue;
        m.csi_of[j] = (u32)m.csi_set.size();
        m.csi_set.push_back(end ? vp.easy_set : writer && h ? vp.writer_set + (n_writers++ / 2) % VOL_WRITER_SETS : hot && h ? pinned : any);
    }
    m.att.assign(std::max<size_t>(m.csi_set.size(), 1) * VOL_MAX_MOUNTS, VOL_NONE);
    return m;
}

struct Problem {
    u32 N, Wn, T, S, n_sc, n_ports;
    std::vector<u64> valid;
    std::vector<i64> cpu, mem;
    std::vector<u32> total;
    std::vector<u64> sc;        // [n_sc][Wn]
    std::vector<RTask> rt;
    std::vector<u64> X;         // [S][Wn]
    std::vector<u32> list_off, list_node, list_svc, list_fail;
    std::vector<u64> portmap;   // [n_ports][Wn]
    std::vector<u32> pset_off, pset_ids;
    i64 UC, UM;
    // feature level 3: generic reservations. n_kinds kinds (ids 1..n_kinds); gcnt[kind][N] the nodes' counts; a task's set names
    // rows of the (kind, value) table sorted by (kind, value) — the engine's batch layout (swp_engine.hip build_batch)
    u32 n_kinds = 0;
    std::vector<int32_t> gcnt;             // [(n_kinds + 1)][N]
    std::vector<u32> tg;                   // [T] set of the task, 0 = none
    std::vector<u32> gs_off, gs_row, rg_kind, rg_k0, rg_k1;
    std::vector<int32_t> rg_val;
    bool lacks(const std::vector<int32_t>& cnt, u32 j, u32 n) const {   // HasEnough fails for one of task j's reservations
        if (tg.empty()) return false;
        for (u32 g = gs_off[tg[j]]; g < gs_off[tg[j] + 1]; ++g)
            if (cnt[(size_t)rg_kind[gs_row[g]] * N + n] < rg_val[gs_row[g]]) return true;
        return false;
    }
};

struct State {   // everything a resolver mutates or emits
    std::vector<i64> cpu, mem;
    std::vector<u32> total;
    std::vector<u64> X, portmap;
    std::vector<u32> list_node, list_svc, list_fail;
    std::vector<int32_t> out, log_prev, last;
    std::vector<u32> log_node, log_task, inf_task, inf_pos;
    std::vector<int32_t> gcnt;
    Ctl ctl{};
};

static Problem make_problem(u32 seed, u32 N, u32 T, u32 S, int order, int feat) {
    std::mt19937_64 g(seed);
    auto rnd = [&](u32 k) { return (u32)(g() % k); };
    Problem p;
    p.N = N;
    p.Wn = (N + 63) / 64;
    p.T = T;
    p.S = S;
    p.UC = 250'000'000;
    p.UM = 256ll << 20;
    p.valid.assign(p.Wn, 0);
    p.cpu.resize(N);
    p.mem.resize(N);
    p.total.resize(N);
    std::vector<u32> zone(N), ssd(N);
    u32 lvl_mode = rnd(4);   // 0: all zero, 1: small spread, 2: wide spread, 3: a few stragglers far below, 4 (EMU_LVL_MODE=4 only): hundreds of levels, 5 (EMU_LVL_MODE=5 only): a tenth of the nodes emptied
    if (const char* lm = getenv("EMU_LVL_MODE")) lvl_mode = (u32)atoi(lm);
    for (u32 n = 0; n < N; ++n) {
        if (rnd(50) != 0) p.valid[n >> 6] |= 1ull << (n & 63);
        p.cpu[n] = (i64)(4 + rnd(60)) * 1'000'000'000 + (rnd(3) ? 0 : rnd(1000));          // not always a multiple of the unit
        p.mem[n] = (i64)(8 + rnd(120)) * (1ll << 30) + (rnd(3) ? 0 : rnd(4096));
        if (rnd(40) == 0) p.cpu[n] = -(i64)rnd(1000);                                       // over-committed node (scheduler.go:378-379)
        p.total[n] = lvl_mode == 0 ? 0 : lvl_mode == 1 ? rnd(3) : lvl_mode == 2 ? rnd(40) : lvl_mode == 4 ? rnd(700) : lvl_mode == 5 ? (rnd(10) ? 10 + rnd(2) : 0) : (rnd(30) ? 20 + rnd(2) : rnd(5));
        zone[n] = rnd(8);
        ssd[n] = rnd(10) < 7;
    }
    // static classes: zone (none / z0..z9) x ssd-only
    p.n_sc = 22;
    p.sc.assign((size_t)p.n_sc * p.Wn, 0);
    for (u32 c = 0; c < p.n_sc; ++c)
        for (u32 n = 0; n < N; ++n) {
            const u32 z = c % 11, s = c / 11;
            bool ok = (p.valid[n >> 6] >> (n & 63)) & 1;
            if (z > 0 && zone[n] != z - 1) ok = false;   // z9, z10 match nothing
            if (s && !ssd[n]) ok = false;
            if (ok) p.sc[(size_t)c * p.Wn + (n >> 6)] |= 1ull << (n & 63);
        }
    // ports
    p.n_ports = 4;
    p.portmap.assign((size_t)p.n_ports * p.Wn, 0);
    for (u32 q = 0; q < p.n_ports; ++q)
        for (u32 n = 0; n < N; ++n)
            if (rnd(10) == 0) p.portmap[(size_t)q * p.Wn + (n >> 6)] |= 1ull << (n & 63);
    p.pset_off = {0, 1, 2, 4};   // three port sets: {0}, {1}, {2,3}
    p.pset_ids = {0, 1, 2, 3};
    // services
    struct Svc { u32 sc, kc, km, flags, pset; u64 maxrep; };
    std::vector<Svc> sv(S);
    for (u32 s = 0; s < S; ++s) {
        Svc& v = sv[s];
        v.sc = rnd(2) ? rnd(p.n_sc) : 0;
        v.flags = rnd(8) ? RT_RES : 0;
        v.kc = (v.flags & RT_RES) ? (1u << rnd(4)) : 0;    // 0.25 .. 2 cores
        v.km = (v.flags & RT_RES) ? (1u << rnd(5)) : 0;    // 256 MiB .. 4 GiB
        if (feat >= 1 && rnd(6) == 0) { v.flags |= RT_RES; v.kc = 40 + rnd(200); v.km = 16 + rnd(300); }   // a heavy service: nodes fill up
        v.pset = 0;
        if (feat >= 2 && rnd(12) == 0) { v.flags |= RT_PORTS; v.pset = rnd(3); }
        v.maxrep = 0;
        if (feat >= 1 && rnd(10) == 0) { v.flags |= RT_MAXREP; v.maxrep = 1 + rnd(3); }
        if (feat >= 2 && rnd(25) == 0) v.flags |= RT_UNCOUNTED;
    }
    // tasks
    p.rt.resize(T);
    std::vector<u32> ntasks(S, 0), rank(T);
    for (u32 j = 0; j < T; ++j) {
        u32 s = order == 0 ? j % S : order == 1 ? std::min<u32>(j / ((T + S - 1) / S), S - 1) : rnd(S);
        RTask& r = p.rt[j];
        memset(&r, 0, sizeof r);
        r.svc = s;
        r.sc = sv[s].sc;
        r.flags = sv[s].flags;
        r.cpu = (i64)sv[s].kc * p.UC;
        r.mem = (i64)sv[s].km * p.UM;
        r.pset = sv[s].pset;
        r.maxrep = sv[s].maxrep;
        rank[j] = ntasks[s]++;
    }
    // exception lists: pre-existing (node, svcCount, failures) entries + one reserved slot per task
    p.X.assign((size_t)S * p.Wn, 0);
    p.list_off.assign(S + 1, 0);
    std::vector<u32> init_cnt(S, 0);
    for (u32 s = 0; s < S; ++s) {
        p.list_off[s] = (u32)p.list_node.size();
        if (feat >= 1 && rnd(3) == 0) {
            std::set<u32> ns;
            u32 k = 1 + rnd(N / 4 + 1);
            for (u32 i = 0; i < k; ++i) ns.insert(rnd(N));
            for (u32 n : ns) {
                if (!((p.valid[n >> 6] >> (n & 63)) & 1)) continue;
                u32 cntv = rnd(4), fl = rnd(5) ? 0 : 5 + rnd(3);
                if (!cntv && !fl) cntv = 1;
                p.list_node.push_back(n);
                p.list_svc.push_back(cntv);
                p.list_fail.push_back(fl);
                p.X[(size_t)s * p.Wn + (n >> 6)] |= 1ull << (n & 63);
            }
        }
        init_cnt[s] = (u32)p.list_node.size() - p.list_off[s];
        for (u32 i = 0; i < ntasks[s]; ++i) {
            p.list_node.push_back(LIST_EMPTY);
            p.list_svc.push_back(0);
            p.list_fail.push_back(0);
        }
    }
    p.list_off[S] = (u32)p.list_node.size();
    for (u32 j = 0; j < T; ++j) p.rt[j].slot = p.list_off[p.rt[j].svc] + init_cnt[p.rt[j].svc] + rank[j];
    if (feat >= 3) {   // generic reservations: 3 kinds, a third of the services reserve one or two of them
        p.n_kinds = 3;
        p.gcnt.assign((size_t)(p.n_kinds + 1) * N, 0);
        for (u32 k = 1; k <= p.n_kinds; ++k)
            for (u32 n = 0; n < N; ++n)
                if (rnd(4)) p.gcnt[(size_t)k * N + n] = (int32_t)rnd(k == 1 ? 4 : 12);   // scarce / plentiful, some nodes offer none
        std::vector<std::vector<std::pair<u32, int32_t>>> svc_set(S);
        std::set<std::pair<u32, int32_t>> pairs;
        for (u32 s = 0; s < S; ++s) {
            if (rnd(3)) continue;
            const u32 k1 = 1 + rnd(p.n_kinds);
            svc_set[s].push_back({k1, (int32_t)(1 + rnd(3))});
            if (rnd(2)) {
                const u32 k2 = 1 + rnd(p.n_kinds);
                if (k2 != k1) svc_set[s].push_back({k2, (int32_t)(1 + rnd(2))});
            }
            std::sort(svc_set[s].begin(), svc_set[s].end());
            for (auto& pr : svc_set[s]) pairs.insert(pr);
        }
        std::map<std::pair<u32, int32_t>, u32> row_of;
        for (auto& pr : pairs) {
            row_of[pr] = (u32)p.rg_kind.size();
            p.rg_kind.push_back(pr.first);
            p.rg_val.push_back(pr.second);
        }
        const u32 R = (u32)p.rg_kind.size();
        p.rg_k0.resize(R);
        p.rg_k1.resize(R);
        for (u32 r = 0; r < R;) {
            u32 q = r;
            while (q < R && p.rg_kind[q] == p.rg_kind[r]) ++q;
            for (u32 x = r; x < q; ++x) { p.rg_k0[x] = r; p.rg_k1[x] = q; }
            r = q;
        }
        p.gs_off.assign(2, 0);
        std::vector<u32> set_of(S, 0);
        for (u32 s = 0; s < S; ++s) {
            if (svc_set[s].empty()) continue;
            set_of[s] = (u32)p.gs_off.size() - 1;
            for (auto& pr : svc_set[s]) p.gs_row.push_back(row_of[pr]);
            p.gs_off.push_back((u32)p.gs_row.size());
        }
        p.tg.assign(T, 0);
        for (u32 j = 0; j < T; ++j) {
            p.tg[j] = set_of[p.rt[j].svc];
            if (p.tg[j]) p.rt[j].flags |= RT_RES;   // ResourceFilter.SetTask: enabled by a generic reservation alone (filter.go:61-74)
        }
    }
    return p;
}

static State initial_state(const Problem& p) {
    State s;
    s.cpu = p.cpu;
    s.mem = p.mem;
    s.total = p.total;
    s.X = p.X;
    s.portmap = p.portmap;
    s.list_node = p.list_node;
    s.list_svc = p.list_svc;
    s.list_fail = p.list_fail;
    s.out.assign(p.T, -1);
    s.log_prev.assign(p.T, -7);
    s.last.assign(p.N, -1);
    s.log_node.assign(p.T, 0);
    s.log_task.assign(p.T, 0);
    s.inf_task.assign(p.T, 0);
    s.inf_pos.assign(p.T, 0);
    s.gcnt = p.gcnt;
    return s;
}

// k_scan's semantics (swp_device.hpp): F = static class & ResourceFilter & ~used host ports, against the state NOW
static void scan_window(const Problem& p, const State& s, u32 j0, u32 cnt, std::vector<u64>& F) {
    F.assign((size_t)cnt * p.Wn, 0);
    for (u32 j = 0; j < cnt; ++j) {
        const RTask& r = p.rt[j0 + j];
        for (u32 w = 0; w < p.Wn; ++w) {
            u64 word = p.sc[(size_t)r.sc * p.Wn + w];
            if (r.flags & RT_RES) {
                u64 fit = 0;
                for (u32 i = 0; i < 64 && w * 64 + i < p.N; ++i)
                    if (r.cpu <= s.cpu[w * 64 + i] && r.mem <= s.mem[w * 64 + i] && !p.lacks(s.gcnt, j0 + j, w * 64 + i)) fit |= 1ull << i;
                word &= fit;
            }
            if (r.flags & RT_PORTS)
                for (u32 q = p.pset_off[r.pset]; q < p.pset_off[r.pset + 1]; ++q) word &= ~s.portmap[(size_t)p.pset_ids[q] * p.Wn + w];
            F[(size_t)j * p.Wn + w] = word;
        }
    }
}

// sequential restatement of one window
static void ref_window(const Problem& p, State& s, u32 j0, u32 cnt, const std::vector<u64>& F, MountRun* mr = nullptr) {
    auto ports_free = [&](const RTask& r, u32 n) {
        for (u32 q = p.pset_off[r.pset]; q < p.pset_off[r.pset + 1]; ++q)
            if ((s.portmap[(size_t)p.pset_ids[q] * p.Wn + (n >> 6)] >> (n & 63)) & 1) return false;
        return true;
    };
    auto commit = [&](const RTask& r, u32 gj, u32 n, u32 e) {
        s.cpu[n] -= r.cpu;
        s.mem[n] -= r.mem;
        if (!p.tg.empty())   // Claim: the count drops by the request
            for (u32 g = p.gs_off[p.tg[gj]]; g < p.gs_off[p.tg[gj] + 1]; ++g) s.gcnt[(size_t)p.rg_kind[p.gs_row[g]] * p.N + n] -= p.rg_val[p.gs_row[g]];
        if (r.flags & RT_PORTS)
            for (u32 q = p.pset_off[r.pset]; q < p.pset_off[r.pset + 1]; ++q) s.portmap[(size_t)p.pset_ids[q] * p.Wn + (n >> 6)] |= 1ull << (n & 63);
        if (!(r.flags & RT_UNCOUNTED)) {
            s.total[n] += 1;
            if (e == LIST_EMPTY) {
                s.X[(size_t)r.svc * p.Wn + (n >> 6)] |= 1ull << (n & 63);
                s.list_node[r.slot] = n;
                s.list_svc[r.slot] = 1;
                s.list_fail[r.slot] = 0;
            } else
                s.list_svc[e] += 1;
        }
        const u32 ci = s.ctl.ncommit++;
        s.log_node[ci] = n;
        s.log_task[ci] = gj;
        s.log_prev[ci] = s.last[n];
        s.last[n] = (int32_t)ci;
        s.out[gj] = (int32_t)n;
        if (mr) mr->placed(gj, n);
    };
    for (u32 j = 0; j < cnt; ++j) {
        const u32 gj = j0 + j;
        const RTask& r = p.rt[gj];
        const u64* f = &F[(size_t)j * p.Wn];
        // plain nodes
        u64 bestk = ~0ull;
        for (u32 n = 0; n < p.N; ++n) {
            if (!((f[n >> 6] >> (n & 63)) & 1)) continue;
            if ((s.X[(size_t)r.svc * p.Wn + (n >> 6)] >> (n & 63)) & 1) continue;
            if ((r.flags & RT_RES) && !(r.cpu <= s.cpu[n] && r.mem <= s.mem[n])) continue;
            if ((r.flags & RT_RES) && p.lacks(s.gcnt, gj, n)) continue;
            if ((r.flags & RT_PORTS) && !ports_free(r, n)) continue;
            if (mr && !mr->passes(gj, n)) continue;
            u64 k = ((u64)s.total[n] << 32) | n;
            if (k < bestk) bestk = k;
        }
        if (bestk != ~0ull) { commit(r, gj, (u32)bestk, LIST_EMPTY); continue; }
        // exception list
        u64 bhi = ~0ull, blo = ~0ull;
        u32 be = 0;
        for (u32 e = p.list_off[r.svc]; e < p.list_off[r.svc + 1]; ++e) {
            u32 n = s.list_node[e];
            if (n == LIST_EMPTY) continue;
            if (!((f[n >> 6] >> (n & 63)) & 1)) continue;
            if ((r.flags & RT_RES) && !(r.cpu <= s.cpu[n] && r.mem <= s.mem[n])) continue;
            if ((r.flags & RT_RES) && p.lacks(s.gcnt, gj, n)) continue;
            if ((r.flags & RT_PORTS) && !ports_free(r, n)) continue;
            if (mr && !mr->passes(gj, n)) continue;
            u32 svc = s.list_svc[e], fl = s.list_fail[e];
            if ((r.flags & RT_MAXREP) && !((u64)svc < r.maxrep)) continue;
            u32 fcl = fl >= MAX_FAILURES ? fl - (MAX_FAILURES - 1) : 0;
            u64 hi = ((u64)fcl << 32) | svc, lo = ((u64)s.total[n] << 32) | n;
            if (hi < bhi || (hi == bhi && lo < blo)) { bhi = hi; blo = lo; be = e; }
        }
        if (bhi != ~0ull) { commit(r, gj, (u32)blo, be); s.ctl.slow_tasks++; continue; }
        if (mr && mr->is(gj)) mr->no_node++;
        s.inf_task[s.ctl.ninf] = gj;
        s.inf_pos[s.ctl.ninf] = s.ctl.ncommit;
        s.ctl.ninf++;
    }
}

template <class V>
static bool same(const char* what, const V& a, const V& b, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (a[i] != b[i]) {
            fprintf(stderr, "MISMATCH %s[%zu]: emu %lld ref %lld\n", what, i, (long long)a[i], (long long)b[i]);
            return false;
        }
    return true;
}


