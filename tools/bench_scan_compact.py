#!/usr/bin/env python3
"""What the compact instance of the scan resolver (csrc/swp_scan.hpp) gives on a cluster of more than 4 096 nodes whose burst is
constrained to a labelled pool, and what its probe costs where it refuses: one JSON line (and --out FILE).

Two libraries in ONE process, on one box, interleaved: the tree's, and --parent PATH (the parent commit's libswp.so, e.g.
tools/_ab/libswp_old.so built as tools/README.md says for gpu_ab.sh). Every figure is the wall time of one whole swp_schedule_batch from
the same saved state (swp_state_save / swp_state_restore between calls), --runs runs (default 3) a side, the sides alternating.

  gain      100 000 one-off tasks, 10 000 nodes, 10 services all constrained to zones z0 .. z2 (service k to zone k % 3; ~3 750 nodes),
            round-robin. Both libraries must return the same out_node and fail_hist (asserted); the gain is ACCEPTED when the tree's
            slowest run beats the parent's fastest.
  refusal   6 services over zones z0 .. z5 (service k to zone k), 20 000 tasks on 6 000 nodes, round-robin: every stretch's union is
            4 431 nodes, every probe refuses. Tree minus parent next to the parent's own spread; the probes are counted in a child
            process that runs the batch once under SWP_DBG=32 (one line per probe on stderr).

  pool      100 000 one-off tasks, 10 000 nodes, 8 services all constrained to zone z0 (1 237 nodes), round-robin: a saturated pool,
            its backlog mostly twins of tasks that found no node. The union's rows fit the LDS of the batched instance's compact form
            (k_scanb<.., true>; scan_lds_bc restated and asserted below), and the tree's library must report scan_batched_tasks > 0
            (asserted). FASTER when the parent's fastest run minus the tree's slowest exceeds the parent's own spread. `gain`'s union
            (3 638 nodes) is too large for it: the same path as before, the two sides within that shape's spread. A union of 1 237
            nodes needs the eight-nodes-a-thread instance, which the launcher takes only under SWP_SCANB_COMPACT=1: the tool sets it
            for this shape (the parent's library does not know it).
  pool_small  the same on 8 000 nodes with 80 000 tasks: zone z0 has 1 002 nodes, four a thread — the launcher's default takes the batched
            form (no knob set; scan_batched_tasks > 0 asserted). FASTER as for `pool`.

usage: python tools/bench_scan_compact.py --parent PATH [--runs 3] [--shapes gain,refusal,pool,pool_small] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from swarmkit_amd import abi, synth, sched as swsched  # noqa: E402
from swarmkit_amd import host as swhost  # noqa: E402


def pools(N, T, zones):
    wl = synth.Workload("cfg3", T=T, N=N, services=len(zones))
    wl.svc_zone = np.array(zones)
    wl.svc_nohdd = np.zeros(len(zones), dtype=bool)
    wl.svc_plat = np.zeros(len(zones), dtype=np.int64)
    return wl


SHAPES = {"gain": lambda: pools(10_000, 100_000, [k % 3 for k in range(10)]), "refusal": lambda: pools(6_000, 20_000, list(range(6))),
          "pool": lambda: pools(10_000, 100_000, [0] * 8), "pool_small": lambda: pools(8_000, 80_000, [0] * 8)}
LDS_BUDGET = 160 * 1024 - 512


def scan_lds_bc(n_c, n_svc, n_sc):
    """csrc/swp_scan.hpp restated: node rows, the two (service, node) matrices and the class rows over the union; the argmins, the
    queue, a window's records and ids, the table of descriptors"""
    return ((n_c * 24 + 15) & ~15) + 2 * n_svc * n_c * 4 + n_sc * ((n_c + 63) // 64) * 8 + 3 * 4 * 8 + (256 // 64) * 8 + 16 + 256 * 64 + 256 * 4 + 1024 * 4


class Side:
    """One library: an engine with the workload loaded and its state saved."""

    def __init__(self, name, lib, wl):
        self.name = name
        self.s = swsched.Scheduler(engine=abi.Engine(lib_path=lib, earlier_stats=name == "parent"))   # (the parent's swp_stats_t may lack the counters appended since)
        self.descs = np.ascontiguousarray(swhost.load_workload(self.s, wl), dtype=abi.TASK_DTYPE)
        self.e = self.s.e
        self.out = np.empty(wl.T, dtype=np.int32)
        self.hist = np.zeros((wl.T, abi.NFILTERS), dtype=np.uint32)
        self.e.state_save()
        self.run()   # warm: modules, pools, the pinned blocks
        self.want_out, self.want_hist = self.out.copy(), self.hist.copy()
        self.stats = self.e.stats()

    def run(self):
        t = time.perf_counter()
        self.e._ck(self.e.L.swp_schedule_batch(self.e.h, self.descs.ctypes.data, len(self.descs), self.out.ctypes.data, self.hist.ctypes.data))
        dt = (time.perf_counter() - t) * 1e3
        self.stats = self.e.stats()
        self.e.state_restore()
        return dt


def summary(xs):
    return {"runs_ms": [round(x, 3) for x in xs], "min": round(min(xs), 3), "median": round(statistics.median(xs), 3), "max": round(max(xs), 3), "spread": round(max(xs) - min(xs), 3)}


def measure(shape, parent, runs):
    wl = SHAPES[shape]()
    sides = [Side("parent", os.path.abspath(parent), wl), Side("tree", abi.build_library(), wl)]
    p, t = sides
    assert (p.want_out == t.want_out).all(), "the two libraries place the batch differently"
    assert (p.want_hist == t.want_hist).all(), "the two libraries explain the batch differently"
    ms = {s.name: [] for s in sides}
    for r in range(runs):
        for s in (sides if r % 2 == 0 else sides[::-1]):
            ms[s.name].append(s.run())
            assert (s.out == s.want_out).all()
    union = int(np.isin(wl.node_zone, sorted(set(int(z) for z in wl.svc_zone))).sum())
    res = {"tasks": wl.T, "nodes": wl.N, "services": wl.S, "order": "rr", "union_nodes": union, "placed": int((t.want_out >= 0).sum()),
           "parent_ms": summary(ms["parent"]), "tree_ms": summary(ms["tree"])}
    for s in sides:
        res[s.name + "_stats"] = {k: int(s.stats[k]) for k in ("scan_tasks", "scan_launches", "resolve_launches", "scan_batched_tasks", "scan_skipped")}
    res["static_classes"] = int(t.stats["last_static_classes"])
    res["scan_lds_bc"] = scan_lds_bc(union, wl.S, res["static_classes"])
    return res


def count_probes(shape):
    """one run of the tree's library under SWP_DBG=32 in a child process: the probes it enqueued"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--probes-of", shape], capture_output=True, text=True, env=dict(os.environ, SWP_DBG="32"), timeout=600)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    return sum(1 for line in r.stderr.splitlines() if "scan probe:" in line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--shapes", default="gain,refusal,pool,pool_small")
    ap.add_argument("--out", default=None)
    ap.add_argument("--probes-of", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.probes_of:
        wl = SHAPES[a.probes_of]()
        s = swsched.Scheduler(engine=abi.Engine(lib_path=abi.build_library()))
        s.e.schedule_batch(np.ascontiguousarray(swhost.load_workload(s, wl), dtype=abi.TASK_DTYPE))
        return
    if not a.parent:
        ap.error("--parent PATH: the parent commit's libswp.so")
    os.environ.pop("SWP_DBG", None)
    os.environ.pop("SWP_SCANB_COMPACT", None)
    out = {"tool": "bench_scan_compact", "runs": a.runs}
    shapes = a.shapes.split(",")
    if "gain" in shapes:
        gain = out["gain"] = measure("gain", a.parent, a.runs)
        gain["probes"] = count_probes("gain")
        gain["accepted"] = gain["tree_ms"]["max"] < gain["parent_ms"]["min"]
        gain["parent_min_over_tree_max"] = round(gain["parent_ms"]["min"] / gain["tree_ms"]["max"], 2)
        assert gain["scan_lds_bc"] > LDS_BUDGET and gain["tree_stats"]["scan_batched_tasks"] == 0, "gain's union is meant to be too large for the batched instance"
    if "refusal" in shapes:
        refusal = out["refusal"] = measure("refusal", a.parent, a.runs)
        refusal["probes"] = count_probes("refusal")
        refusal["tree_minus_parent_median_ms"] = round(refusal["tree_ms"]["median"] - refusal["parent_ms"]["median"], 3)
    for shape, knob in (("pool", "1"), ("pool_small", None)):
        if shape not in shapes:
            continue
        if knob:
            os.environ["SWP_SCANB_COMPACT"] = knob
        try:
            pool = out[shape] = measure(shape, a.parent, a.runs)
            pool["probes"] = count_probes(shape)
        finally:
            os.environ.pop("SWP_SCANB_COMPACT", None)
        pool["SWP_SCANB_COMPACT"] = knob
        assert pool["scan_lds_bc"] <= LDS_BUDGET, "the pool's rows must fit the batched instance's LDS: fewer services"
        assert pool["tree_stats"]["scan_batched_tasks"] > 0, "no stretch of the pool went through the batched instance"
        pool["faster"] = pool["parent_ms"]["min"] - pool["tree_ms"]["max"] > pool["parent_ms"]["spread"]
        pool["parent_min_over_tree_max"] = round(pool["parent_ms"]["min"] / pool["tree_ms"]["max"], 2)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
