// swp_resolve6.hip — translation unit of the block resolver (k_r6_*, swp_resolve6.hpp) and its launchers.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "swp_launch.hpp"
#include "swp_wave.hpp"
#define SWP_R6_KERNELS
#define SWP_VOL_KERNELS
#include "swp_resolve6.hpp"
#include "swp_resolve7.hpp"
#include "swp_rounds.hpp"
#include "swp_fitpairs.hpp"
#define SWP_ENF_KERNELS
#include "swp_enforce.hpp"
#define SWP_SCAN_KERNELS
#include "swp_scan.hpp"

namespace swpdev {

// the host rule's figures (swp_rounds.hpp knows no kernel header) are the kernels'
static_assert(R6_RING_TASKS == R6_RING && R6_RING_LIST == R6_LIST_RING && R6_RING_BLOCK == R6_BMAX, "swp_rounds.hpp and swp_resolve6.hpp disagree on the ring");
#if R6_RING_ON
#define R6_COMMIT_RING_KERNEL k_r6_commit_r
#define R6_PROPOSE_RING_KERNEL k_r6_propose_r
#define R6_PROPOSE_SMALL_RING_KERNEL k_r6_propose_small_r
#define R6_PROPOSE_TINY_RING_KERNEL k_r6_propose_tiny_r
#else   // (never launched: launch_r6_rounds refuses R6Args.ring in a build without the ring)
#define R6_COMMIT_RING_KERNEL k_r6_commit
#define R6_PROPOSE_RING_KERNEL k_r6_propose
#define R6_PROPOSE_SMALL_RING_KERNEL k_r6_propose_small
#define R6_PROPOSE_TINY_RING_KERNEL k_r6_propose_tiny
#endif

size_t r6_propose_lds_size(uint32_t n_words) { return r6_propose_lds(n_words); }
size_t r6_commit_lds_size(uint32_t n_words, uint32_t block, uint32_t n_rr, bool compact, uint32_t win) { return r6_commit_lds(n_words, block, n_rr, compact, win); }
size_t r6_commit_lds_ring_size(uint32_t n_words, uint32_t block, uint32_t n_rr, uint32_t ring, uint32_t win) { return r6_commit_lds_ring(n_words, block, n_rr, ring, win); }
uint32_t r6_block_max() { return R6_FLAT_BMAX; }
uint32_t r6_ring_block_max() { return R6_BMAX; }
uint32_t r7_block_max() { return R7_BMAX; }

// base / highest level, then level planes + demand-class rows from the node rows as they are
hipError_t launch_r6_build(const R6Args& a, hipStream_t s) {
    hipLaunchKernelGGL(k_r6_minmax, dim3(1), dim3(1024), 256, s, a);
    hipLaunchKernelGGL(k_r6_rows, dim3((a.n_words + 3) / 4), dim3(256), 0, s, a);
    return hipGetLastError();
}

// `rounds` rounds of propose + commit; a round past the end of the stretch is a no-op
hipError_t launch_r6_rounds(const R6Args& a, uint32_t rounds, hipStream_t s, int dev) {
    const bool cpt = a.compact != 0 && !a.csi_of;   // (a batch with cluster mounts has its own commit instance, without the index)
    // a ring round (R6Args.ring): the plain instance's only, with the long lists, and a block the kernels' arrays are sized for
    if (a.ring && (!R6_RING_ON || cpt || a.csi_of || !a.ext || a.ring != R6_RING || a.block > R6_BMAX)) return hipErrorInvalidValue;
    if (!a.ring && a.block > R6_FLAT_BMAX) return hipErrorInvalidValue;   // (the flat instances' twin count ends there)
    const size_t lp = r6_propose_lds(a.n_words);
    const size_t lc = a.ring ? r6_commit_lds_ring(a.n_words, a.block, a.n_dc + a.n_dm, a.ring, a.win) : r6_commit_lds(a.n_words, a.block, a.n_dc + a.n_dm, cpt, a.win);
    hipError_t r;
    if (lp > 48 * 1024 && (r = ensure_big_lds(reinterpret_cast<const void*>(cpt ? &k_r6_propose_c : a.ring ? &R6_PROPOSE_RING_KERNEL : &k_r6_propose), dev)) != hipSuccess) return r;
    if (lc > 48 * 1024 && (r = ensure_big_lds(reinterpret_cast<const void*>(cpt ? &k_r6_commit_c : a.csi_of ? &k_r6_commit_v : a.ring ? &R6_COMMIT_RING_KERNEL : &k_r6_commit), dev)) != hipSuccess) return r;
    // compact == 2: k_r6_commit_c builds the next round's index at its end; a launch of k_r6_compact only in front of the chunk's first round
    // (the state may have moved since the last commit: a scan stretch, a rebuild). Task-rows mode builds the rows the index pass reads
    // at the START of a round: there the index keeps its own launch.
    const bool fused = cpt && a.compact == 2 && !a.task_rows;
    R6Args ac = a;
    if (cpt && !fused) ac.compact = 1;
    for (uint32_t i = 0; i < rounds; ++i) {
        if (a.task_rows) hipLaunchKernelGGL(k_r6_taskrows, dim3((a.n_words + 3) / 4, (a.block + 63) / 64), dim3(256), (size_t)a.block * 16, s, a);
        if (a.csi_of) hipLaunchKernelGGL(k_r6_volrows, dim3((a.n_words + 255) / 256, a.block), dim3(256), 0, s, a);   // (batches with cluster mounts only)
        if (cpt) {   // rounds with a compact index of the level their first task aims at (run_blocks decides when)
            if (!fused || i == 0) hipLaunchKernelGGL(k_r6_compact, dim3(1), dim3(1024), 256, s, ac);
            if (a.n_words <= R6_SMALL_WORDS) hipLaunchKernelGGL(k_r6_propose_small_c, dim3(a.block), dim3(64 * R6_PW), lp, s, ac);
            else hipLaunchKernelGGL(k_r6_propose_c, dim3(a.block), dim3(64 * R6_PW), lp, s, ac);
            hipLaunchKernelGGL(k_r6_commit_c, dim3(1), dim3(R6_COMMIT_THREADS), lc, s, ac);
            continue;
        }
        if (a.ring) {   // the ring rounds' instances, chosen as the flat ones below
            if (a.n_words <= R6_TINY_WORDS && a.block > 1024u) hipLaunchKernelGGL(R6_PROPOSE_TINY_RING_KERNEL, dim3(a.block), dim3(64 * R6_PW_TINY), lp, s, a);
            else if (a.n_words <= R6_SMALL_WORDS) hipLaunchKernelGGL(R6_PROPOSE_SMALL_RING_KERNEL, dim3(a.block), dim3(64 * R6_PW), lp, s, a);
            else hipLaunchKernelGGL(R6_PROPOSE_RING_KERNEL, dim3(a.block), dim3(64 * R6_PW), lp, s, a);
        } else if (a.n_words <= R6_TINY_WORDS && a.block > 1024u) hipLaunchKernelGGL(k_r6_propose_tiny,   // (up to 1 024 workgroups of eight waves are resident together as they are)
             dim3(a.block), dim3(64 * R6_PW_TINY), lp, s, a);
        else if (a.n_words <= R6_SMALL_WORDS) hipLaunchKernelGGL(k_r6_propose_small, dim3(a.block), dim3(64 * R6_PW), lp, s, a);   // (LDS of 8 chunks: never beyond 48 KB)
        else hipLaunchKernelGGL(k_r6_propose, dim3(a.block), dim3(64 * R6_PW), lp, s, a);
        if (a.csi_of) hipLaunchKernelGGL(k_r6_commit_v, dim3(1), dim3(R6_COMMIT_THREADS), lc, s, a);
        else if (a.ring) hipLaunchKernelGGL(R6_COMMIT_RING_KERNEL, dim3(1), dim3(R6_COMMIT_THREADS), lc, s, a);
        else hipLaunchKernelGGL(k_r6_commit, dim3(1), dim3(R6_COMMIT_THREADS), lc, s, a);
    }
    return hipGetLastError();
}

// ---- CSI volumes (swp_volumes.hpp) ----
hipError_t launch_vol_topology(const VolTopoArgs& a, hipStream_t s) {
    if (a.n_vol == 0 || a.n_nodes == 0) return hipSuccess;
    for (uint32_t v0 = 0; v0 < a.n_vol; v0 += 65535u) {   // (grid.y is a 16-bit quantity)
        VolTopoArgs c = a;
        c.vol0 = v0;
        hipLaunchKernelGGL(k_vol_topology, dim3((a.n_words * 64 + 255) / 256, std::min<uint32_t>(65535u, a.n_vol - v0)), dim3(256), 0, s, c);
    }
    return hipGetLastError();
}
hipError_t launch_vol_choose(const VolChooseArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_vol_choose, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}

// the preassigned pair pass (swp_fitpairs.hpp), without and with cluster mounts: one thread per node segment
hipError_t launch_fit_pairs(const FitArgs& a, hipStream_t s) {
    if (a.n_seg == 0) return hipSuccess;
    hipLaunchKernelGGL(k_fit_pairs, dim3((a.n_seg + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_fit_pairs_vol(const FitVolArgs& a, hipStream_t s) {
    if (a.f.n_seg == 0) return hipSuccess;
    hipLaunchKernelGGL(k_fit_pairs_vol, dim3((a.f.n_seg + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

// the enforcer sweep's nodes with a generic task (swp_enforce.hpp): one wave per node, four to a workgroup
hipError_t launch_enforce_generic(const EnfGenArgs& a, hipStream_t s) {
    if (a.n_gen == 0) return hipSuccess;
    hipLaunchKernelGGL(k_enforce_generic, dim3((a.n_gen + 3) / 4), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---- node-range shards with the rounds on the device (swp_resolve7.hpp) ----
size_t r7_commit_lds_size(uint32_t hw_total, uint32_t block, uint32_t n_rr) { return r7_commit_lds(hw_total, block, n_rr); }
// `args`: device array of the argument records of the `count` shards that live on device `dev` (all of the same block size; the
// launch geometry is sized for the largest of them)
hipError_t launch_r7_propose(const R6Args* args, uint32_t count, uint32_t block, uint32_t max_words, bool task_rows, bool csi, hipStream_t s, int dev) {
    const size_t lp = r6_propose_lds(max_words);
    hipError_t r;
    if (lp > 48 * 1024 && (r = ensure_big_lds(reinterpret_cast<const void*>(&k_r7_propose), dev)) != hipSuccess) return r;
    if (task_rows) hipLaunchKernelGGL(k_r7_taskrows, dim3((max_words + 3) / 4, count), dim3(256), (size_t)block * 16, s, args);
    if (csi) hipLaunchKernelGGL(k_r7_volrows, dim3((max_words + 255) / 256, block, count), dim3(256), 0, s, args);   // (batches with cluster mounts only)
    if (max_words <= R6_SMALL_WORDS) hipLaunchKernelGGL(k_r7_propose_small, dim3(block, count), dim3(64 * R6_PW), lp, s, args);   // (LDS of 8 chunks: never beyond 48 KB)
    else hipLaunchKernelGGL(k_r7_propose, dim3(block, count), dim3(64 * R6_PW), lp, s, args);
    return hipGetLastError();
}
// fold + match + apply: one workgroup per shard of the device; `m`: the job's shard table in device memory
hipError_t launch_r7_commit(const R6Args* args, uint32_t count, const R7Args* m, size_t lds, bool csi, uint32_t shard0, hipStream_t s, int dev) {
    hipError_t r;
    if (lds > 48 * 1024 && (r = ensure_big_lds(reinterpret_cast<const void*>(csi ? &k_r7_commit_v : &k_r7_commit), dev)) != hipSuccess) return r;
    if (csi) hipLaunchKernelGGL(k_r7_commit_v, dim3(count), dim3(R6_COMMIT_THREADS), lds, s, args, m, shard0);
    else hipLaunchKernelGGL(k_r7_commit, dim3(count), dim3(R6_COMMIT_THREADS), lds, s, args, m, shard0);
    return hipGetLastError();
}


hipError_t launch_r7_settle(const R6Args* args, uint32_t count, const R7Args* m, uint32_t shard0, hipStream_t s) {
    hipLaunchKernelGGL(k_r7_settle, dim3(count), dim3(64), 0, s, args, m, shard0);
    return hipGetLastError();
}

// ---- the scan resolver (swp_scan.hpp): a stretch of tasks one after the other, every task by one workgroup over all nodes ----
uint32_t scan_max_nodes() { return SCAN_MAXN; }
template <int NQ, bool LM>
static hipError_t launch_scan_as(const ScanArgs& s, size_t lds, hipStream_t st, int dev) {
    hipError_t r;
    if (lds > 48 * 1024 && (r = ensure_big_lds(reinterpret_cast<const void*>(&k_scan<NQ, LM>), dev)) != hipSuccess) return r;
    hipLaunchKernelGGL((k_scan<NQ, LM>), dim3(1), dim3(SCAN_THREADS), lds, st, s);
    return hipGetLastError();
}
template <bool LM>
static hipError_t launch_scan_nq(const ScanArgs& s, size_t lds, hipStream_t st, int dev) {
    switch (scan_nq(s.a.n_nodes)) {
        case 1: return launch_scan_as<1, LM>(s, lds, st, dev);
        case 2: return launch_scan_as<2, LM>(s, lds, st, dev);
        default: return launch_scan_as<4, LM>(s, lds, st, dev);
    }
}
bool scan_batched_fits(uint32_t n_nodes, uint32_t n_svc, uint32_t n_sc) { return !getenv("SWP_SCAN_UNBATCHED") && scan_lds_b(n_nodes, n_svc, n_sc) <= (size_t)160 * 1024 - 512; }
bool scan_matrices_in_lds(uint32_t n_nodes, uint32_t n_svc) { return scan_lds_lm(n_nodes, n_svc) <= (size_t)160 * 1024 - 512; }
template <int NQ>
static hipError_t launch_scanb_as(const ScanArgs& s, size_t lds, hipStream_t st, int dev) {
    hipError_t r;
    if (lds > 48 * 1024 && (r = ensure_big_lds(reinterpret_cast<const void*>(&k_scanb<NQ>), dev)) != hipSuccess) return r;
    hipLaunchKernelGGL((k_scanb<NQ>), dim3(1), dim3(SCANB_THREADS), lds, st, s);
    return hipGetLastError();
}
// node_local: no task of the stretch reserves generic resources, publishes host ports or mounts cluster volumes (the caller looked) —
// then, when everything a task reads fits in LDS, SCAN_B tasks share a barrier (k_scanb)
hipError_t launch_scan(const ScanArgs& s, hipStream_t st, int dev, bool node_local) {
    hipLaunchKernelGGL(k_scan_fill, dim3(1024), dim3(256), 0, st, s);
    hipLaunchKernelGGL(k_scan_lists, dim3(64, s.n_svc), dim3(256), 0, st, s);
    if (node_local && scan_batched_fits(s.a.n_nodes, s.n_svc, s.n_sc)) {
        const size_t lds = scan_lds_b(s.a.n_nodes, s.n_svc, s.n_sc);
        switch (scanb_nq(s.a.n_nodes)) {
            case 1: return launch_scanb_as<1>(s, lds, st, dev);
            case 2: return launch_scanb_as<2>(s, lds, st, dev);
            case 4: return launch_scanb_as<4>(s, lds, st, dev);
            case 8: return launch_scanb_as<8>(s, lds, st, dev);
            default: return launch_scanb_as<16>(s, lds, st, dev);
        }
    }
    // the (service, node) matrices in LDS when they fit next to the node rows: a task's turn then waits for no global load
    if (scan_matrices_in_lds(s.a.n_nodes, s.n_svc)) return launch_scan_nq<true>(s, scan_lds_lm(s.a.n_nodes, s.n_svc), st, dev);
    return launch_scan_nq<false>(s, scan_lds(s.a.n_nodes), st, dev);
}

// the matrices alone (what the spread instance, swp_scan_spread.hip, runs on)
hipError_t launch_scan_matrices(const ScanArgs& s, hipStream_t st) {
    hipLaunchKernelGGL(k_scan_fill, dim3(1024), dim3(256), 0, st, s);
    hipLaunchKernelGGL(k_scan_lists, dim3(64, s.n_svc), dim3(256), 0, st, s);
    return hipGetLastError();
}

// ... over the union's n_c columns, behind launch_scan_probe (the compact spread instance; n_c may be 0: nothing to fill)
hipError_t launch_scan_matrices_compact(const ScanArgs& s, hipStream_t st) {
    hipLaunchKernelGGL(k_scan_fill_c, dim3(1024), dim3(256), 0, st, s);
    hipLaunchKernelGGL(k_scan_lists_c, dim3(64, s.n_svc), dim3(256), 0, st, s);
    return hipGetLastError();
}

// ---- the compact instance: a cluster beyond SCAN_MAXN nodes, a stretch whose class rows' union is not ----
// the probe: which class rows the tasks [j0, j1) name, their union, its node count (*s.cnc: the caller reads it), prefix sums and map
hipError_t launch_scan_probe(const ScanArgs& s, hipStream_t st) {
    hipError_t r = hipMemsetAsync(s.cused, 0, (size_t)s.n_sc * 4, st);
    if (r != hipSuccess) return r;
    hipLaunchKernelGGL(k_scan_mark, dim3(std::min<uint32_t>(64u, (s.j1 - s.j0 + 255u) / 256u)), dim3(256), 0, st, s);
    hipLaunchKernelGGL(k_scan_union, dim3(1), dim3(SCAN_THREADS), scan_union_lds(), st, s);
    return hipGetLastError();
}
template <int NQ, bool LM>
static hipError_t launch_scan_c_as(const ScanArgs& s, size_t lds, hipStream_t st, int dev) {
    hipError_t r;
    if (lds > 48 * 1024 && (r = ensure_big_lds(reinterpret_cast<const void*>(&k_scan<NQ, LM, true>), dev)) != hipSuccess) return r;
    hipLaunchKernelGGL((k_scan<NQ, LM, true>), dim3(1), dim3(SCAN_THREADS), lds, st, s);
    return hipGetLastError();
}
template <bool LM>
static hipError_t launch_scan_c_nq(const ScanArgs& s, size_t lds, hipStream_t st, int dev) {
    switch (scan_nq(s.n_c)) {
        case 1: return launch_scan_c_as<1, LM>(s, lds, st, dev);
        case 2: return launch_scan_c_as<2, LM>(s, lds, st, dev);
        default: return launch_scan_c_as<4, LM>(s, lds, st, dev);
    }
}
// The ONE rule for a compact stretch (the driver asks it, the launcher launches by it). Its rows over the union must fit in LDS; beyond
// that the batched form is taken by default only for unions of at most SCANB_COMPACT_AUTO nodes — up to four nodes a thread, where a
// batch's evaluation is what it is on the dense batch. Measured (profiles/scanb_compact.json): a pool of 1 237 nodes needs the
// eight-nodes-a-thread instance and lost 9 ms of 73 to the one-task-a-barrier instance. SWP_SCANB_COMPACT=1: every union that fits
// (tests, A/B runs), =0: none.
#define SCANB_COMPACT_AUTO 1024u
bool scan_batched_fits_c(uint32_t n_c, uint32_t n_svc, uint32_t n_sc) {
    if (getenv("SWP_SCAN_UNBATCHED") || scan_lds_bc(n_c, n_svc, n_sc) > (size_t)160 * 1024 - 512) return false;
    const char* env = getenv("SWP_SCANB_COMPACT");
    return env ? atoi(env) != 0 : n_c <= SCANB_COMPACT_AUTO;
}
template <int NQ>
static hipError_t launch_scanb_c_as(const ScanArgs& s, size_t lds, hipStream_t st, int dev) {
    hipError_t r;
    if (lds > 48 * 1024 && (r = ensure_big_lds(reinterpret_cast<const void*>(&k_scanb<NQ, true>), dev)) != hipSuccess) return r;
    hipLaunchKernelGGL((k_scanb<NQ, true>), dim3(1), dim3(SCANB_THREADS), lds, st, s);
    return hipGetLastError();
}
// the stretch behind a probe that found s.n_c <= SCAN_MAXN nodes: matrices of n_c columns, and over them the batched instance where
// the stretch is node_local (launch_scan) and its rows over n_c nodes fit in LDS, the one-task-a-barrier instance otherwise
hipError_t launch_scan_compact(const ScanArgs& s, hipStream_t st, int dev, bool node_local) {
    if (s.n_c == 0 || s.n_c > SCAN_MAXN) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_scan_fill_c, dim3(1024), dim3(256), 0, st, s);
    hipLaunchKernelGGL(k_scan_lists_c, dim3(64, s.n_svc), dim3(256), 0, st, s);
    if (node_local && scan_batched_fits_c(s.n_c, s.n_svc, s.n_sc)) {
        const size_t lds = scan_lds_bc(s.n_c, s.n_svc, s.n_sc);
        switch (scanb_nq(s.n_c)) {
            case 1: return launch_scanb_c_as<1>(s, lds, st, dev);
            case 2: return launch_scanb_c_as<2>(s, lds, st, dev);
            case 4: return launch_scanb_c_as<4>(s, lds, st, dev);
            case 8: return launch_scanb_c_as<8>(s, lds, st, dev);
            default: return launch_scanb_c_as<16>(s, lds, st, dev);
        }
    }
    if (scan_matrices_in_lds(s.n_c, s.n_svc)) return launch_scan_c_nq<true>(s, scan_lds_lm(s.n_c, s.n_svc), st, dev);
    return launch_scan_c_nq<false>(s, scan_lds(s.n_c), st, dev);
}

}  // namespace swpdev
