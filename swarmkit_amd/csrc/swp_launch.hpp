// swp_launch.hpp — what the engine runtime (swp_engine.hip) and the resolver translation units share on the host side.
#pragma once
#include <hip/hip_runtime.h>

#include "swp_types.hpp"

namespace swpdev {

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a per-DEVICE setting: remembered per (kernel, device ordinal), so
// that a process holding engines on several GPUs (a manager sharding over the node's 8 devices) raises the limit on each.
hipError_t ensure_big_lds(const void* fn, int device);

// k_resolve6, the block resolver (swp_resolve6.hip)
struct R6Args;
size_t r6_propose_lds_size(uint32_t n_words);
size_t r6_commit_lds_size(uint32_t n_words, uint32_t block, uint32_t n_rr, bool compact = false, uint32_t win = 0);   // win: R6Args.win   // compact: with the room for a compact index (k_r6_compact)
size_t r6_commit_lds_ring_size(uint32_t n_words, uint32_t block, uint32_t n_rr, uint32_t ring, uint32_t win = 0);   // ... of a ring round (R6Args.ring)
uint32_t r6_ring_block_max();   // the largest block of a ring round (R6_BMAX)
uint32_t r6_block_max();   // the largest flat block of a single engine ...
uint32_t r7_block_max();   // ... and of the node-range shards
// Tasks per round of the block resolver unless SWP_R6_BLOCK says otherwise. A single engine: as many 64-task groups as the commit
// kernel's LDS holds (windows of R6_WIN list entries a task: 1 408 tasks next to the TK row of 10 000 nodes); the shards, whose commit
// kernel holds whole folded lists: 768 as far as the LDS allows.
#define R6_BLOCK_DEFAULT_CAP 2048u
#define R7_BLOCK_DEFAULT_CAP 768u
hipError_t launch_r6_build(const R6Args& a, hipStream_t s);
hipError_t launch_r6_rounds(const R6Args& a, uint32_t rounds, hipStream_t s, int dev);

// CSI volumes (swp_volumes.hpp, built in swp_resolve6.hip)
struct VolTopoArgs;
struct VolChooseArgs;
hipError_t launch_vol_topology(const VolTopoArgs& a, hipStream_t s);
hipError_t launch_vol_choose(const VolChooseArgs& a, hipStream_t s);
// the preassigned pair pass (swp_fitpairs.hpp, built in swp_resolve6.hip): a call without a mount template, and one with
struct FitArgs;
struct FitVolArgs;
hipError_t launch_fit_pairs(const FitArgs& a, hipStream_t s);          // k_fit_pairs
hipError_t launch_fit_pairs_vol(const FitVolArgs& a, hipStream_t s);   // k_fit_pairs_vol

// the enforcer sweep's nodes with a generic task (swp_enforce.hpp, built in swp_resolve6.hip): one wave per node
struct EnfGenArgs;
hipError_t launch_enforce_generic(const EnfGenArgs& a, hipStream_t s);

// node-range shards, rounds on the device (swp_resolve7.hpp, built in swp_resolve6.hip)
struct R7Args;
size_t r7_commit_lds_size(uint32_t hw_total, uint32_t block, uint32_t n_rr);
hipError_t launch_r7_propose(const R6Args* args, uint32_t count, uint32_t block, uint32_t max_words, bool task_rows, bool csi, hipStream_t s, int dev);
hipError_t launch_r7_commit(const R6Args* args, uint32_t count, const R7Args* m, size_t lds, bool csi, uint32_t shard0, hipStream_t s, int dev);   // fold + match + apply
hipError_t launch_r7_settle(const R6Args* args, uint32_t count, const R7Args* m, uint32_t shard0, hipStream_t s);   // the last round's volume reservations, to every shard

// sharded scan, host-merged rounds (swp_shard.hip)
struct ProposeArgs;
struct ShardApplyArgs;
hipError_t launch_propose(const ProposeArgs& a, hipStream_t s);
hipError_t launch_shard_apply(const ShardApplyArgs& a, hipStream_t s);

// the scan resolver (swp_scan.hpp, built in swp_resolve6.hip)
struct ScanArgs;
uint32_t scan_max_nodes();
bool scan_batched_fits(uint32_t n_nodes, uint32_t n_svc, uint32_t n_sc);   // k_scanb (several tasks a barrier, identical unplaceable tasks skipped) can take such a batch: everything it reads fits in LDS
hipError_t launch_scan(const ScanArgs& s, hipStream_t st, int dev, bool node_local);
hipError_t launch_scan_probe(const ScanArgs& s, hipStream_t st);                // the compact instance: the union of the stretch's class rows, *s.cnc its node count
bool scan_batched_fits_c(uint32_t n_c, uint32_t n_svc, uint32_t n_sc);          // ... k_scanb's compact form takes a node-local stretch over a union of n_c nodes: its rows fit in LDS and the union is small enough (or SWP_SCANB_COMPACT=1)
hipError_t launch_scan_compact(const ScanArgs& s, hipStream_t st, int dev, bool node_local);   // ... and the stretch over it (s.n_c as read from the probe, <= scan_max_nodes()); node_local: as for launch_scan
hipError_t launch_scan_matrices(const ScanArgs& s, hipStream_t st);             // k_scan_fill + k_scan_lists alone: the (service, node) matrices over all nodes
// its spread instance: one-off tasks with spread preferences (swp_scan_spread.hpp, built in swp_scan_spread.hip)
struct SpreadArgs;
size_t scan_spread_lds_size(uint32_t n_nodes, uint32_t max_ntn, uint32_t max_depth, uint32_t n_trees, uint32_t tot_ntn);   // the kernel's LDS for these node slots, the largest / deepest tree and all trees' tables
hipError_t launch_scan_spread(const SpreadArgs& p, hipStream_t st, int dev);    // behind launch_scan_matrices
hipError_t launch_scan_matrices_compact(const ScanArgs& s, hipStream_t st);     // k_scan_fill_c + k_scan_lists_c alone: the matrices over the union's s.n_c columns (behind launch_scan_probe)
// the compact spread instance, behind launch_scan_probe + launch_scan_matrices_compact: k_spread_base (the pairs' leaf sums over the nodes outside the union) + k_scan_spread<.., true>
hipError_t launch_scan_spread_compact(const SpreadArgs& p, const uint32_t* pair_svc, const uint32_t* pair_tree, uint32_t* base, hipStream_t st, int dev);
// the wide spread instance (k_scan_spread_wide): all node slots of a nodeSet beyond scan_max_nodes(), the node rows in global memory
size_t scan_spread_wide_lds_size(uint32_t max_ntn, uint32_t max_depth, uint32_t n_trees, uint32_t tot_ntn);   // its LDS: no node rows
uint32_t scan_spread_wide_max_nodes();                                               // SPREAD_WIDE_MAXN: the key's 16 bits for the node
hipError_t launch_scan_spread_wide(const SpreadArgs& p, hipStream_t st, int dev);    // behind launch_scan_matrices
// a compact spread segment whose union is too wide: the pieces to cut it into (k_spread_cut, swp_scan_spread.hpp), one workgroup
struct CutArgs;
hipError_t launch_spread_cut(CutArgs p, hipStream_t st, int dev);

// task groups (swp_groups.hip)
struct Groups2Args;
hipError_t launch_groups2(const Groups2Args& a, hipStream_t s, int dev);
struct G2Pub;
hipError_t launch_groups2_streamed(const Groups2Args& a, const G2Pub& pb, hipStream_t s, int dev);   // k_groups2s

// runs of identical tasks (swp_waterfill.hip)
struct WaterArgs;
hipError_t launch_waterfill(const WaterArgs& a, hipStream_t s);

}  // namespace swpdev
