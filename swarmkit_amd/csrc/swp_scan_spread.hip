// swp_scan_spread.hip — translation unit of k_scan_spread (swp_scan_spread.hpp) and its launcher. A unit of its own: the scan
// resolver's shipped instances (swp_resolve6.hip) are compiled without it.
#include <hip/hip_runtime.h>

#include "swp_launch.hpp"
#include "swp_wave.hpp"
#include "swp_resolve6.hpp"
#define SWP_SCAN_SPREAD_KERNEL
#include "swp_scan_spread.hpp"

namespace swpdev {

size_t scan_spread_lds_size(uint32_t n_nodes, uint32_t max_ntn, uint32_t max_depth, uint32_t n_trees, uint32_t tot_ntn) { return scan_lds_sp(n_nodes, max_ntn, max_depth, n_trees, tot_ntn); }

template <int NQ>
static hipError_t launch_scan_spread_as(const SpreadArgs& p, size_t lds, hipStream_t st, int dev) {
    hipError_t r;
    if (lds > 48 * 1024 && (r = ensure_big_lds(reinterpret_cast<const void*>(&k_scan_spread<NQ>), dev)) != hipSuccess) return r;
    hipLaunchKernelGGL((k_scan_spread<NQ>), dim3(1), dim3(SCAN_THREADS), lds, st, p);
    return hipGetLastError();
}
// the tasks [p.s.j0, p.s.j1) one after the other; p.s.hmat / emat as launch_scan_matrices left them
hipError_t launch_scan_spread(const SpreadArgs& p, hipStream_t st, int dev) {
    const size_t lds = scan_lds_sp(p.s.a.n_nodes, p.max_ntn, p.max_depth, p.n_trees, p.tot_ntn);
    if (p.s.a.n_nodes == 0 || p.s.a.n_nodes > SCAN_MAXN || lds > (size_t)160 * 1024 - 512) return hipErrorInvalidValue;
    switch (scan_nq(p.s.a.n_nodes)) {
        case 1: return launch_scan_spread_as<1>(p, lds, st, dev);
        case 2: return launch_scan_spread_as<2>(p, lds, st, dev);
        default: return launch_scan_spread_as<4>(p, lds, st, dev);
    }
}

// ---- the compact instance: a nodeSet beyond SCAN_MAXN slots, a segment whose class rows' union is not
template <int NQ>
static hipError_t launch_scan_spread_c_as(const SpreadArgs& p, size_t lds, hipStream_t st, int dev) {
    hipError_t r;
    if (lds > 48 * 1024 && (r = ensure_big_lds(reinterpret_cast<const void*>(&k_scan_spread<NQ, true>), dev)) != hipSuccess) return r;
    hipLaunchKernelGGL((k_scan_spread<NQ, true>), dim3(1), dim3(SCAN_THREADS), lds, st, p);
    return hipGetLastError();
}
// behind launch_scan_probe of [p.s.j0, p.s.j1) (p.s.n_c as read from it, 0 included: every task is left without a node) and
// launch_scan_matrices_compact: the pairs' base sums from the lists as they are, then the tasks one after the other
hipError_t launch_scan_spread_compact(const SpreadArgs& p, const uint32_t* pair_svc, const uint32_t* pair_tree, uint32_t* base, hipStream_t st, int dev) {
    const size_t lds = scan_lds_sp(p.s.n_c, p.max_ntn, p.max_depth, p.n_trees, p.tot_ntn);
    if (p.s.n_c > SCAN_MAXN || p.n_pairs == 0 || lds > (size_t)160 * 1024 - 512) return hipErrorInvalidValue;
    hipError_t r = hipMemsetAsync(base, 0, (size_t)p.n_pairs * p.max_ntn * 4, st);
    if (r != hipSuccess) return r;
    hipLaunchKernelGGL(k_spread_base, dim3(64, p.n_pairs), dim3(256), 0, st, p, pair_svc, pair_tree, base);
    switch (scan_nq(p.s.n_c)) {
        case 1: return launch_scan_spread_c_as<1>(p, lds, st, dev);
        case 2: return launch_scan_spread_c_as<2>(p, lds, st, dev);
        default: return launch_scan_spread_c_as<4>(p, lds, st, dev);
    }
}

// ---- the wide instance: all node slots of a nodeSet beyond SCAN_MAXN, the node rows in global memory (k_scan_spread_wide)
size_t scan_spread_wide_lds_size(uint32_t max_ntn, uint32_t max_depth, uint32_t n_trees, uint32_t tot_ntn) { return scan_lds_spw(max_ntn, max_depth, n_trees, tot_ntn); }
uint32_t scan_spread_wide_max_nodes() { return SPREAD_WIDE_MAXN; }
// the tasks [p.s.j0, p.s.j1) one after the other; p.s.hmat / emat as launch_scan_matrices left them, over all nodes
hipError_t launch_scan_spread_wide(const SpreadArgs& p, hipStream_t st, int dev) {
    const size_t lds = scan_lds_spw(p.max_ntn, p.max_depth, p.n_trees, p.tot_ntn);
    if (p.s.a.n_nodes == 0 || p.s.a.n_nodes > SPREAD_WIDE_MAXN || lds > (size_t)160 * 1024 - 512) return hipErrorInvalidValue;
    hipError_t r;
    if (lds > 48 * 1024 && (r = ensure_big_lds(reinterpret_cast<const void*>(&k_scan_spread_wide), dev)) != hipSuccess) return r;
    hipLaunchKernelGGL(k_scan_spread_wide, dim3(1), dim3(SCAN_THREADS), lds, st, p);
    return hipGetLastError();
}

// ---- a compact segment too wide for the kernel: where to cut it (k_spread_cut), one workgroup
// the piece's union in LDS where it fits next to the flags, else in p.cu; hipErrorInvalidValue: not even the flags fit (the caller refuses)
hipError_t launch_spread_cut(CutArgs p, hipStream_t st, int dev) {
    if (p.j0 >= p.j1 || p.max_pieces == 0 || p.n_sc == 0) return hipErrorInvalidValue;
    p.u_lds = spread_cut_lds(p.n_sc, p.n_words, true) <= (size_t)160 * 1024 - 512 ? 1u : 0u;
    const size_t lds = spread_cut_lds(p.n_sc, p.n_words, p.u_lds != 0);
    if (lds > (size_t)160 * 1024 - 512 || (!p.u_lds && !p.cu)) return hipErrorInvalidValue;
    hipError_t r;
    if (lds > 48 * 1024 && (r = ensure_big_lds(reinterpret_cast<const void*>(&k_spread_cut), dev)) != hipSuccess) return r;
    hipLaunchKernelGGL(k_spread_cut, dim3(1), dim3(SCAN_THREADS), lds, st, p);
    return hipGetLastError();
}

}  // namespace swpdev
