// swp_fitpairs.hpp — the records of the preassigned pair pass (swp_fit_pairs / swp_fit_pairs_volumes) and its kernel for
// calls with cluster mounts, k_fit_pairs_vol. The kernel for calls without mounts, k_fit_pairs, lives in swp_device.hpp and is built
// with the engine; this one needs the volume device functions (swp_volumes.hpp) and is built with them in swp_resolve6.hip.
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

#ifdef SWP_VOL_KERNELS
// ---------------------------------------------------------------------------------------------
// k_fit_pairs_vol — k_fit_pairs (swp_device.hpp) for a call in which some template has cluster mounts: the same chain per node
// segment, then VolumesFilter (filter.go:424-432) as the pipeline's last entry and, on a pass of all eight, chooseTaskVolumes
// (scheduler.go:663-677). taskFitNode chooses and reserves nothing, so the volume state is read-only for the whole pass: segments
// stay independent, one thread per segment as in k_fit_pairs. A pair whose choice fails is not booked on its node; its row keeps
// the prefix the mounts in front of the failing one chose. The thread writes its pairs' rows and nothing else of the volumes.
// ---------------------------------------------------------------------------------------------
WV_KERNEL(256) void k_fit_pairs_vol(FitVolArgs av) {
    const FitArgs& a = av.f;
    const u32 s = wv::block() * 256u + wv::tid();
    if (s >= a.n_seg) return;
    const u32 n = a.seg_node[s], w = n >> 6;
    const u64 bit = 1ull << (n & 63);
    const bool ready = (a.ready[w] & bit) != 0;
    i64 cpu = a.cpu[n], mem = a.mem[n];
    u32 total = a.total[n];
    const u32 p1 = a.seg_off[s + 1];
    for (u32 p = a.seg_off[s]; p < p1; ++p) {
        const FitPair q = a.pairs[p];
        const FitTmpl& t = a.tm[q.tmpl];
        const u32 fl = t.rt.flags;
        int ff = -1;
        if (!ready) ff = 0;
        else if ((fl & RT_RES) && !(t.rt.cpu <= cpu && t.rt.mem <= mem)) ff = 1;
        else if ((fl & RT_RES) && [&] {
                     for (u32 g = 0; g < t.n_gen; ++g)
                         if (a.gcnt[(size_t)a.gkind[t.gen_off + g] * a.gstride + n] < a.gval[t.gen_off + g]) return true;   // HasEnough, validate.go:24-52
                     return false;
                 }())
            ff = 1;
        else if (t.rt.cls_plug && !(a.plug[(size_t)t.rt.cls_plug * a.n_words + w] & bit)) ff = 2;
        else if (t.rt.cls_con && !(a.con[(size_t)t.rt.cls_con * a.n_words + w] & bit)) ff = 3;
        else if (t.rt.cls_plat && !(a.plat[(size_t)t.rt.cls_plat * a.n_words + w] & bit)) ff = 4;
        else if ((fl & RT_PORTS) && [&] {
                     for (u32 k = 0; k < t.n_ports; ++k)
                         if (a.port_taken[a.port_slot[q.port_off + k]]) return true;   // HostPortFilter, filter.go:335-350
                     return false;
                 }())
            ff = 5;
        else if ((fl & RT_MAXREP) && !((u64)a.svc_cnt[q.svc_slot] < t.rt.maxrep)) ff = 6;
        else if (t.mset && (av.vol.n_vol == 0 || !((vol_filter_word(av.vol, t.mset, w) >> (n & 63u)) & 1ull))) ff = 7;   // VolumesFilter, the pipeline's last entry
        u32* row = av.att + (size_t)q.idx * VOL_MAX_MOUNTS;
        if (ff == -1 && t.mset) {
            if (vol_choose(av.vol, t.mset, n, row, nullptr) == 0) ff = FIT_FF_NO_VOLUME;   // (the row: the chosen prefix, VOL_NONE from the failing mount on)
        } else {
            for (u32 m = 0; m < VOL_MAX_MOUNTS; ++m) row[m] = VOL_NONE;
        }
        a.out[q.idx] = ff;
        if (ff != -1) continue;
        // NodeInfo.addTask (nodeinfo.go:128-154), as k_fit_pairs books it
        cpu -= t.rt.cpu;
        mem -= t.rt.mem;
        for (u32 g = 0; g < t.n_gen; ++g) {
            int32_t* c = a.gcnt + (size_t)a.gkind[t.gen_off + g] * a.gstride + n;
            *c = max(*c - a.gval[t.gen_off + g], 0);
        }
        if (!(fl & RT_UNCOUNTED)) {
            ++total;
            ++a.svc_cnt[q.svc_slot];
        }
        for (u32 k = 0; k < t.n_ports; ++k) a.port_taken[a.port_slot[q.port_off + k]] = 1u;
    }
    a.cpu[n] = cpu;
    a.mem[n] = mem;
    a.total[n] = total;
}
#endif   // SWP_VOL_KERNELS

}  // namespace swpdev
