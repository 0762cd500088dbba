// swp_publish.hpp — k_publish: the decided prefix of a running batch, handed to the host while later rounds run.
//
// The resolvers decide tasks strictly in order: everything in front of Blk6.pos (the next undecided task) is final, and so is a
// run k_waterfill has finished. The streamed driver (swp_engine.hip, swp_batch_run_streamed) enqueues this kernel behind every few
// rounds, every scan stretch and every k_waterfill run. It copies out_node[published .. pos) into a host-visible array (fine-grained
// pinned memory: device stores land in host DRAM, no copy engine, no stream synchronisation), and then tells the host how far it got:
// it appends `pos` — a MARK — to a ring in the same pinned block and bumps the mark counter.
//
// Ordering: every thread stores its share with plain vector stores and issues a SYSTEM-scope release fence (agent scope ends at this
// device's L2: the host is outside it); the workgroup barrier orders all of those in front of lane 0, which stores the mark and then
// the counter with a system-scope release store. A host that reads the counter with an acquire load therefore finds the mark and every
// placement in front of it. The host does not rely on that alone: it pre-fills the array with PUB_SENTINEL, which no placement can
// equal, and refuses a range that still holds one.
//
// One workgroup: a publish moves a few thousand dwords. `published` and the mark count live in device memory (the kernel never reads
// the host's copy back over the bus).
#pragma once
#include <hip/hip_runtime.h>

#include "swp_types.hpp"

namespace swpdev {

#define PUB_THREADS 256
#define PUB_SENTINEL ((int32_t)0x80000000)   // neither -1 ("no suitable node") nor a node index

struct PubArgs {
    const u32* pos;          // device: the resolvers' next undecided task (Blk6.pos); nullptr: `upto` says how far the batch is decided
    u32 upto;
    u32 n_tasks;
    u32 ring;                // entries of h_ring
    const int32_t* out;      // device [n_tasks]: out_node as the resolvers write it
    u32* state;              // device [2]: tasks published so far, marks appended so far
    int32_t* h_pub;          // host-visible [n_tasks]
    u32* h_ring;             // host-visible [ring]: the marks, in order
    u32* h_count;            // host-visible: marks appended so far
};

hipError_t launch_publish(const PubArgs& a, hipStream_t s);   // swp_publish.hip

#ifdef SWP_PUBLISH_KERNEL
__global__ __launch_bounds__(PUB_THREADS) void k_publish(PubArgs a) {
    const u32 from = a.state[0];
    u32 pos = a.pos ? *a.pos : a.upto;
    if (pos > a.n_tasks) pos = a.n_tasks;
    if (pos < from) pos = from;   // (a stretch that starts where a run ended: never backwards)
    for (u32 i = from + threadIdx.x; i < pos; i += PUB_THREADS) a.h_pub[i] = a.out[i];
    __threadfence_system();
    __syncthreads();   // every thread has read state[0] and released its stores
    if (threadIdx.x == 0) {
        const u32 c = a.state[1];
        __hip_atomic_store(&a.h_ring[c % a.ring], pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(a.h_count, c + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        a.state[0] = pos;
        a.state[1] = c + 1u;
    }
}
#endif

}  // namespace swpdev
