// swp_types.hpp — plain C++ records shared by the kernels (swp_device.hpp, swp_resolve6.hpp, ...), the engine runtime
// (swp_engine.hip) and the CPU emulation harnesses (tests/emu/). No HIP types in here.
#pragma once
#include <stdint.h>

namespace swpdev {

typedef unsigned long long u64;
typedef long long i64;
typedef uint32_t u32;

#define DEV_VALID 0x80000000u   // node slot is present in the nodeSet

// mirror of SWP_NODE_* (include/swp.h)
#define NF_READY 0x001u
#define NF_HAS_DESC 0x002u
#define NF_HAS_PLATFORM 0x004u
#define NF_HAS_ENGINE 0x008u
#define NF_HAS_LABELS 0x010u
#define NF_HAS_ELABELS 0x020u
#define NF_MANAGER 0x040u
#define NF_HAS_LOGPLUG 0x080u
#define NF_IP_VALID 0x100u
#define NF_IP_V4 0x200u

// RTask.flags
#define RT_RES 0x1u        // resource filter enabled
#define RT_PORTS 0x2u      // host-port filter enabled
#define RT_MAXREP 0x4u     // max-replicas filter enabled
#define RT_UNCOUNTED 0x8u  // DesiredState > COMPLETED: placement does not bump the task counts
// The task's demand classes (index into the batch's sorted distinct cpu / memory reservations, R6Args.thr in the block
// resolver) ride in the flag word. Meaningful only with RT_RES.
#define RT_DC_SHIFT 8
#define RT_DM_SHIFT 20
#define RT_DCLS_MASK 0xFFFu   // 12 bits each: up to 4 095 distinct cpu and 4 095 distinct memory reservations per batch

#define LIST_EMPTY 0xFFFFFFFFu
#define KEY_NONE 0xFFFFFFFFFFFFFFFFull
#define MAX_FAILURES 5u   // scheduler.go:23

struct RTask {   // 64 B per task, batch order
    i64 cpu, mem;
    u32 flags;
    u32 sc;        // static class (ready & plugin & constraint & platform bitmap row)
    u32 svc;       // batch-local service index
    u32 slot;      // absolute index of this task's own entry in the per-service exception list
    u32 pset;      // batch-local port set
    u32 cls_con, cls_plat, cls_plug;   // batch-local class rows (0 = filter disabled) — explain pass
    u64 maxrep;
    u32 kc, km;    // unused padding (no kernel reads them): keeps the record at 64 B with the offsets the kernels read
};
static_assert(sizeof(RTask) == 64, "RTask layout");

struct DevConstraint {   // 48 B
    u32 kind, op, col, value;
    u32 ip[4];
    u32 ip_kind, prefix_len, ip_is_v4, pad;
};

struct Ctl {
    u32 ncommit, ninf, error, resume;   // resume: first task NOT processed when `error` stopped a resolver (host continues from there)
    u64 verify_retries, slow_tasks, rebases, generic_tasks, spin_waits, pad1;
    u64 cyc[8];   // dbg&16: cycles spent in resolver sections
    u64 m_cyc[4];       // k_groups2's section timers (SWP_G2_PROF build, SWP_DBG=16): inside the walk
    u64 l_cyc[8];       // k_groups2's section timers: further sections
    u64 wave_cyc[16];   // k_groups2's section timers: per-section counts and cycles (admission, sort, candidate batches)
};

enum { ERR_NONE = 0, ERR_LEVEL_RANGE = 1, ERR_GROUP_RANGE = 2 };

}  // namespace swpdev
