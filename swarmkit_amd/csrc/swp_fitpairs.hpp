// swp_fitpairs.hpp — Pipeline.Process for one (task, node) pair and NodeInfo.addTask for a passing one, as device functions every pair
// kernel shares (k_check_pair in swp_device.hpp; k_fit_pairs and k_fit_pairs_vol here), the records of the preassigned pair pass
// (swp_fit_pairs / swp_fit_pairs_volumes) and its two kernels: one segment walk, instantiated without and with cluster
// mounts. The kernels need the volume device functions (swp_volumes.hpp) and are built with them in swp_resolve6.hip.
#pragma once
#include "swp_types.hpp"
#include "swp_volumes.hpp"

namespace swpdev {

struct FitTmpl {
    RTask rt;                 // the template's record (build_batch): classes, reservations, flags, MaxReplicas
    u32 gen_off, n_gen;       // its generic reservations: gkind / gval[gen_off .. +n_gen)
    u32 n_ports, mset;        // ports in its port set: a pair's port slots are port_slot[pair.port_off .. +n_ports); its mount set (0: no cluster
                              // mounts; read by k_fit_pairs_vol only)
};
static_assert(sizeof(FitTmpl) == 80, "FitTmpl layout");
struct FitPair { u32 idx, tmpl, svc_slot, port_off; };   // idx: the pair's position in the caller's array
struct FitArgs {
    u32 n_seg, n_words, gstride, pad;
    const u32* seg_node;      // [n_seg]
    const u32* seg_off;       // [n_seg + 1] into pairs
    const FitPair* pairs;
    const FitTmpl* tm;
    const u32* gkind;
    const int32_t* gval;
    const u32* port_slot;
    u32* port_taken;          // per (segment, port): 1 = held on the node (its initial value: HostNode.ports)
    u32* svc_cnt;             // per (segment, service): ActiveTasksCountByService (initial value: HostNode.svc)
    const u64* ready;
    const u64* con;
    const u64* plat;
    const u64* plug;
    i64* cpu;
    i64* mem;
    u32* total;
    int32_t* gcnt;            // [kind][gstride]
    int32_t* out;             // first failing filter per pair, caller's order; -1 = passed (and applied)
};

// first_fail of a pair that passed all eight filters and for which chooseTaskVolumes found no volume for a mount (include/swp.h
// SWP_FIT_NO_VOLUME): not assigned, not booked (scheduler.go:668-675)
#define FIT_FF_NO_VOLUME 8
struct FitVolArgs {
    FitArgs f;
    VolView vol;              // n_vol == 0: no volume exists, VolumesFilter fails every mount template
    u32* att;                 // [pairs][VOL_MAX_MOUNTS], caller's order: swp_batch_attachments' rows
};

// ---------------------------------------------------------------------------------------------
// fit_first_fail — Pipeline.Process on one (task, node) pair (pipeline.go:56-103): the index of the first failing filter — 0 Ready,
// 1 Resource, 2 Plugin, 3 Constraint, 4 Platform, 5 HostPort, 6 MaxReplicas — or -1. The callers differ in where the node's mutable
// state lives: cpu / mem come by value (global memory or the registers of a segment walk), `port_busy()` and `svc_count()` are asked
// only when every filter in front has passed (a value the host evaluated, or loads from a segment's slots). So is the generic loop.
// ---------------------------------------------------------------------------------------------
template <class PortBusy, class SvcCount>
__device__ inline int fit_first_fail(const RTask& rt, u32 n, u32 n_words, bool ready, i64 cpu, i64 mem, u32 n_gen, const u32* gkind, const int32_t* gval,
                                     const int32_t* gcnt, u32 gstride, const u64* plug, const u64* con, const u64* plat, PortBusy port_busy, SvcCount svc_count) {
    const u32 w = n >> 6;
    const u64 bit = 1ull << (n & 63);
    if (!ready) return 0;
    if (rt.flags & RT_RES) {
        if (!(rt.cpu <= cpu && rt.mem <= mem)) return 1;
        for (u32 g = 0; g < n_gen; ++g)
            if (gcnt[(size_t)gkind[g] * gstride + n] < gval[g]) return 1;   // HasEnough, validate.go:24-52
    }
    if (rt.cls_plug && !(plug[(size_t)rt.cls_plug * n_words + w] & bit)) return 2;
    if (rt.cls_con && !(con[(size_t)rt.cls_con * n_words + w] & bit)) return 3;
    if (rt.cls_plat && !(plat[(size_t)rt.cls_plat * n_words + w] & bit)) return 4;
    if ((rt.flags & RT_PORTS) && port_busy()) return 5;   // HostPortFilter, filter.go:335-350
    if ((rt.flags & RT_MAXREP) && !((u64)svc_count() < rt.maxrep)) return 6;
    return -1;
}

// NodeInfo.addTask (nodeinfo.go:128-154) for a pair that passed, what a placement of swp_schedule_batch books: cpu / mem / total are the
// segment walk's registers, the generic counts, the service count and the port claims the slots in memory
__device__ inline void fit_book(const FitArgs& a, const FitPair& q, const FitTmpl& t, u32 n, i64& cpu, i64& mem, u32& total) {
    cpu -= t.rt.cpu;
    mem -= t.rt.mem;
    for (u32 g = 0; g < t.n_gen; ++g) {
        int32_t* c = a.gcnt + (size_t)a.gkind[t.gen_off + g] * a.gstride + n;
        *c = max(*c - a.gval[t.gen_off + g], 0);   // (an entry that reaches 0 leaves the list)
    }
    if (!(t.rt.flags & RT_UNCOUNTED)) {
        ++total;
        ++a.svc_cnt[q.svc_slot];
    }
    for (u32 k = 0; k < t.n_ports; ++k) a.port_taken[a.port_slot[q.port_off + k]] = 1u;
}

#ifdef SWP_VOL_KERNELS
// ---------------------------------------------------------------------------------------------
// fit_walk — taskFitNode for many preassigned tasks (processPreassignedTasks, scheduler.go:398-426, 646-690). The pairs come grouped by
// node (segments, pair order kept inside each); one thread walks one segment in order and judges every pair with fit_first_fail
// against the node as the earlier passing pairs of the segment left it (fit_book between two tasks): cpu / mem / total in registers,
// the generic counts, host-port claims and per-service counts in slots of its own. Different nodes are independent. The thread is the
// only writer of its node, its slots and its pairs' verdicts: plain loads and stores.
// (the host passes present nodes only: DEV_VALID is set for every one of them, k_check_pair's -2 cannot happen here)
//
// MOUNTS: some template of the call has cluster mounts. Then VolumesFilter (filter.go:424-432) is the pipeline's last entry and, on a
// pass of all eight, chooseTaskVolumes (scheduler.go:663-677) fills the pair's attachment row. taskFitNode chooses and reserves
// nothing, so the volume state is read-only for the whole pass and the segments stay independent. A pair whose choice fails is not
// booked on its node; its row keeps the prefix the mounts in front of the failing one chose. The thread writes its pairs' rows and
// nothing else of the volumes. Without MOUNTS neither `vol` nor `att` is looked at.
// ---------------------------------------------------------------------------------------------
template <bool MOUNTS>
WV_DEV void fit_walk(const FitArgs& a, const VolView* vol, u32* att) {
    const u32 s = wv::block() * 256u + wv::tid();
    if (s >= a.n_seg) return;
    const u32 n = a.seg_node[s];
    const bool ready = (a.ready[n >> 6] >> (n & 63)) & 1ull;
    i64 cpu = a.cpu[n], mem = a.mem[n];
    u32 total = a.total[n];
    const u32 p1 = a.seg_off[s + 1];
    for (u32 p = a.seg_off[s]; p < p1; ++p) {
        const FitPair q = a.pairs[p];
        const FitTmpl& t = a.tm[q.tmpl];
        int ff = fit_first_fail(
            t.rt, n, a.n_words, ready, cpu, mem, t.n_gen, a.gkind + t.gen_off, a.gval + t.gen_off, a.gcnt, a.gstride, a.plug, a.con, a.plat,
            [&] {
                for (u32 k = 0; k < t.n_ports; ++k)
                    if (a.port_taken[a.port_slot[q.port_off + k]]) return true;
                return false;
            },
            [&] { return a.svc_cnt[q.svc_slot]; });
        if constexpr (MOUNTS) {
            if (ff == -1 && t.mset && (vol->n_vol == 0 || !((vol_filter_word(*vol, t.mset, n >> 6) >> (n & 63u)) & 1ull))) ff = 7;
            u32* row = att + (size_t)q.idx * VOL_MAX_MOUNTS;
            if (ff == -1 && t.mset) {
                if (vol_choose(*vol, t.mset, n, row, nullptr) == 0) ff = FIT_FF_NO_VOLUME;   // (the row: the chosen prefix, VOL_NONE from the failing mount on)
            } else {
                for (u32 m = 0; m < VOL_MAX_MOUNTS; ++m) row[m] = VOL_NONE;
            }
        }
        a.out[q.idx] = ff;
        if (ff == -1) fit_book(a, q, t, n, cpu, mem, total);
    }
    a.cpu[n] = cpu;
    a.mem[n] = mem;
    a.total[n] = total;
}
// a call without a mount template: no VolView among the arguments, no attachment row written
WV_KERNEL(256) void k_fit_pairs(FitArgs a) { fit_walk<false>(a, nullptr, nullptr); }
WV_KERNEL(256) void k_fit_pairs_vol(FitVolArgs av) { fit_walk<true>(av.f, &av.vol, av.att); }
#endif   // SWP_VOL_KERNELS

}  // namespace swpdev
