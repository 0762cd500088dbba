// swp_enforce.hpp — the constraint enforcer's sweep, constraintenforcer.rejectNoncompliantTasks (constraint_enforcer.go:65-202), on the
// device: the records of swp_enforce / swp_enforce_generic, the per-task step both kernels share, and k_enforce_generic.
//
// A node none of whose tasks holds AssignedGenericResources is one thread of k_enforce (swp_device.hpp). A node with such a task is
// one WAVE of k_enforce_generic: the walk over its tasks is wave-uniform (cpu, mem and the constraint bit are lane-invariant; the
// step is enf_step, the same function k_enforce calls), and the 64 lanes hold the node's copy of Description.Resources.Generic,
// one list entry a lane, in list order:
//   HasResource (validate.go:54-85) for one assignment entry is three ballots over the entries — same kind and still there; of
//     those, Discrete; of those, Named with the assignment's name — and a first-set-bit rule: a Discrete assignment is decided by the
//     FIRST entry of its kind (it must be Discrete and hold at least the value), a Named one by its first equal name, which must lie
//     in front of the kind's first Discrete entry.
//   ConsumeNodeResources (helpers.go:58-111) is every lane for itself: its entry against the task's assignment entries in order.
// A list of more than 64 entries runs in chunks of 64 over the node's slice of a mutable copy of the lists (`work`); a shorter one
// never leaves the registers. The wave is the only reader and writer of its slice and of its tasks' verdicts: plain loads and
// stores, no atomics. The first assignment that is no longer there rejects its task and ends the node (`break loop`, :196-199):
// every later task of the node gets 0.
//
// Written against swp_wave.hpp only (tests/emu/emu_enforce.cpp runs this source on CPU fibers).
#pragma once
#include "swp_types.hpp"

namespace swpdev {

struct EnfNode { u32 node, first, count, pad; i64 cpu, mem; };
struct EnfTask { i64 cpu, mem; u32 cls_con, flags, desired, state; };
static_assert(sizeof(EnfNode) == 32 && sizeof(EnfTask) == 32, "enforcer record layout");
#define TASK_STATE_ASSIGNED 192u
#define TASK_STATE_COMPLETE 576u

#define ENF_SKIP 0u     // desired / observed state: not looked at (:118-126)
#define ENF_REJECT 1u   // constraints (:162-168) or reservations (:172-184): rejected, `continue` — nothing is claimed
#define ENF_KEEP 2u     // kept: its reservations are off cpu / mem; its generic assignments are looked at next (:186-200)

// one task of the walk, up to line 184 of the reference; `w` / `bit`: the node's word and bit in the class bitmap rows
__device__ inline u32 enf_step(const EnfTask& tk, const u64* __restrict__ con, u32 n_words, u32 w, u64 bit, i64& cpu, i64& mem) {
    if (tk.desired < TASK_STATE_ASSIGNED || tk.desired > TASK_STATE_COMPLETE) return ENF_SKIP;   // :118-120
    if (tk.state >= TASK_STATE_COMPLETE) return ENF_SKIP;                                        // :124-126
    if (tk.cls_con && !(con[(size_t)tk.cls_con * n_words + w] & bit)) return ENF_REJECT;         // :162-168
    if (tk.flags & 1u) {                                                                         // :172-184
        if (tk.mem > mem) return ENF_REJECT;
        if (tk.cpu > cpu) return ENF_REJECT;
        mem -= tk.mem;
        cpu -= tk.cpu;
    }
    return ENF_KEEP;
}

#define ENF_NAMED 1u   // EnfRes.flags: NamedResourceSpec, value = the caller's id of the string (else DiscreteResourceSpec, value = its Value)
#define ENF_GONE 2u    // ... in `work` and in the lanes only: ConsumeNodeResources took the entry off the list
struct EnfRes { u32 kind, flags; i64 value; };   // include/swp.h swp_enforce_res
static_assert(sizeof(EnfRes) == 16, "enforcer resource record layout");

struct EnfGenArgs {
    u32 n_gen, n_words;
    const EnfNode* nodes;        // [n_gen] the nodes with a generic task
    const u32* src;              // [n_gen] a node's position in the caller's array: its list is node_res[node_res_off[src] .. node_res_off[src + 1])
    const EnfTask* tasks;
    const u64* con;              // [classes][n_words]
    const u32* node_res_off;
    const EnfRes* node_res;      // read only
    EnfRes* work;                // a copy of node_res the waves of lists longer than 64 entries mutate (null: no list is that long)
    const u32* task_res_off;     // [tasks + 1]
    const EnfRes* task_res;
    unsigned char* out;
};

#ifdef SWP_ENF_KERNELS
// a wave-uniform read-only record, 64 bits at a time (wv::uload: the scalar cache)
template <class T>
WV_DEV T enf_uload(const T* p) {
    static_assert(sizeof(T) % 8 == 0 && alignof(T) == 8, "records of 64-bit words");
    u64 wd[sizeof(T) / 8];
    WV_UNROLL
    for (u32 k = 0; k < sizeof(T) / 8; ++k) wd[k] = wv::uload(reinterpret_cast<const u64*>(p) + k);
    T out;
    __builtin_memcpy(&out, wd, sizeof(T));
    return out;
}

// HasResource for the assignment entry `ta` over ONE chunk of the list, lane = entry: 0 = this chunk holds no entry that decides
// (go on to the next one; list exhausted: false), 1 = true, 2 = false
WV_DEV u32 enf_has_chunk(const EnfRes& ta, const EnfRes& L) {
    const bool same = !(L.flags & ENF_GONE) && L.kind == ta.kind;
    const u64 m_same = wv::ballot(same);
    if (m_same == 0) return 0;
    const u64 m_disc = wv::ballot(same && !(L.flags & ENF_NAMED));
    if (!(ta.flags & ENF_NAMED)) {   // the first entry of the kind decides (validate.go:66-73: a Named entry returns false for a Discrete assignment)
        const u32 first = (u32)wv::ffs64(m_same);
        if (!((m_disc >> first) & 1ull)) return 2;
        const i64 have = (i64)wv::readlane64((u64)L.value, first);
        return ta.value <= have ? 1u : 2u;
    }
    const u64 m_eq = wv::ballot(same && (L.flags & ENF_NAMED) && L.value == ta.value);
    const u32 f_disc = m_disc ? (u32)wv::ffs64(m_disc) : 64u, f_eq = m_eq ? (u32)wv::ffs64(m_eq) : 64u;
    if (f_eq < f_disc) return 1;   // other names in front of it are passed over (:79-81)
    return f_disc < 64u ? 2u : 0u;
}

// ConsumeNodeResources for this lane's entry against the task's assignment entries [q0, q1), read wave-uniformly
WV_DEV void enf_consume(EnfRes& L, const EnfRes* __restrict__ task_res, u32 q0, u32 q1) {
    for (u32 q = q0; q < q1; ++q) {
        const EnfRes r = enf_uload(task_res + q);
        if ((L.flags & ENF_GONE) || L.kind != r.kind) continue;   // (a removed entry meets no further assignment: helpers.go:76 `break`)
        if (!(r.flags & ENF_NAMED)) {
            if (L.flags & ENF_NAMED) continue;                    // type change, ignore (helpers.go:92-95)
            L.value = (i64)((u64)L.value - (u64)r.value);         // (Go's int64 wraps)
            if (L.value <= 0) L.flags |= ENF_GONE;
        } else if ((L.flags & ENF_NAMED) && L.value == r.value)
            L.flags |= ENF_GONE;
    }
}

WV_KERNEL(256) void k_enforce_generic(EnfGenArgs a) {
    const u32 g = wv::block() * 4u + wv::wave();
    if (g >= a.n_gen) return;   // (the whole wave)
    const u32 lane = wv::lane();
    const EnfNode nd = enf_uload(a.nodes + g);
    const u32 src = wv::uload(a.src + g);
    const u32 r0 = wv::uload(a.node_res_off + src), r1 = wv::uload(a.node_res_off + src + 1);
    const u32 n_chunks = (r1 - r0 + 63u) / 64u;
    const u32 w = nd.node >> 6;
    const u64 bit = 1ull << (nd.node & 63);
    const EnfRes none{0u, ENF_GONE, 0};
    EnfRes reg = none;   // the whole list when it fits the wave
    if (n_chunks == 1 && r0 + lane < r1) reg = a.node_res[r0 + lane];
    i64 cpu = nd.cpu, mem = nd.mem;
    const u32 t1 = nd.first + nd.count;
    for (u32 t = nd.first; t < t1; ++t) {
        const EnfTask tk = enf_uload(a.tasks + t);
        const u32 step = enf_step(tk, a.con, a.n_words, w, bit, cpu, mem);
        const u32 q0 = wv::uload(a.task_res_off + t), q1 = wv::uload(a.task_res_off + t + 1);
        if (step != ENF_KEEP || q0 == q1) {   // (an empty assignment list behaves like nil)
            if (lane == 0) a.out[t] = step == ENF_REJECT ? 1 : 0;
            continue;
        }
        bool there = true;   // every assignment entry is still on the node (:188-194)
        for (u32 q = q0; q < q1 && there; ++q) {
            const EnfRes ta = enf_uload(a.task_res + q);
            u32 v = 0;
            if (n_chunks == 1) v = enf_has_chunk(ta, reg);
            else
                for (u32 c = 0; c < n_chunks && v == 0; ++c) {
                    const u32 i = r0 + c * 64u + lane;
                    v = enf_has_chunk(ta, i < r1 ? a.work[i] : none);
                }
            there = v == 1;
        }
        if (!there) {   // rejected, and `break loop` (:196-199): nobody behind it is looked at
            if (lane == 0) a.out[t] = 1;
            for (u32 u = t + 1 + lane; u < t1; u += 64u) a.out[u] = 0;
            return;
        }
        if (lane == 0) a.out[t] = 0;
        if (n_chunks == 1) enf_consume(reg, a.task_res, q0, q1);   // ClaimResources against the node's copy (:200)
        else
            for (u32 c = 0; c < n_chunks; ++c) {
                const u32 i = r0 + c * 64u + lane;
                EnfRes L = i < r1 ? a.work[i] : none;
                enf_consume(L, a.task_res, q0, q1);
                if (i < r1) a.work[i] = L;
            }
    }
}
#endif   // SWP_ENF_KERNELS

}  // namespace swpdev
