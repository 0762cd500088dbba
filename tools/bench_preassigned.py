#!/usr/bin/env python3
"""processPreassignedTasks at global-service scale: N nodes x S global services (one preassigned task per node each), one JSON line.

  host_all_fit_ms     swp_sched_process_preassigned over all N*S pending tasks, every one fits (the first pass after a global
                      service is created)
  host_first_ms       the same with about 20 % of the nodes too small: those tasks fail and stay pending
  host_recheck_ms     the next call, which checks those pending tasks again (the reference does this before every tick)
  fit_pairs_ms        the engine call alone: swp_fit_pairs over the N*S (node, template) pairs
  loop_ms             ... against swp_check_node + swp_commit per pair on a twin engine (measured over the first --loop-pairs pairs,
                      scaled to all of them: loop_us_per_pair)

--mounts all|alternate gives the services' tasks one cluster mount on a `group:` volume (every service; every second one) and orders the
pending list node by node, so that mount tasks and plain tasks alternate in it: an engine without swp_fit_pairs_volumes ends a run at every
mount task. The engine call is then swp_fit_pairs_volumes and the loop adds swp_choose_volumes.

--lib PATH runs the host-layer figures against another build of libswp.so (an older commit's, for a same-box "before"); a library
without swp_fit_pairs takes the per-task path and the engine-call figures are left out.

usage: python tools/bench_preassigned.py [--nodes 10000] [--services 1 4] [--reps 3] [--mounts none|all|alternate] [--lib PATH]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from swarmkit_amd import abi, sched as swsched  # noqa: E402

RUNNING, PENDING, READY = 512, 64, 2
MOUNTS = "none"   # --mounts


def mounts_of(k):
    return MOUNTS == "all" or (MOUNTS == "alternate" and k % 2 == 1)


def node_doc(i, small):
    return {"ID": "n%06d" % i, "Spec": {"Annotations": {"Name": "node%d" % i, "Labels": {"zone": "z%d" % (i % 4)}}, "Availability": 0},
            "Status": {"State": READY, "Addr": "10.%d.%d.%d" % (i >> 16, (i >> 8) & 255, i & 255)},
            "Description": {"Hostname": "h%d" % i, "Platform": {"Architecture": "amd64", "OS": "linux"},
                            "Resources": {"NanoCPUs": 10**8 if small else 64 * 10**9, "MemoryBytes": 256 << 30},
                            **({} if MOUNTS == "none" else {"CSIInfo": [{"PluginName": "csi-a", "NodeID": "c%d" % i}]})}}


def task_doc(k, i):
    spec = {"Resources": {"Reservations": {"NanoCPUs": 10**9 // 4, "MemoryBytes": 1 << 28}},
            "Placement": {"Constraints": ["node.labels.zone!=nowhere"], "Platforms": [{"Architecture": "amd64", "OS": "linux"}]}}
    if mounts_of(k):
        spec["Container"] = {"Mounts": [{"Type": "CLUSTER", "Source": "group:g", "Target": "/data"}]}
    tid = "g%02d-%06d" % (k, i) if MOUNTS == "none" else "t%06d-%02d" % (i, k)   # (pending tasks are walked in ascending ID)
    return {"ID": tid, "ServiceID": "gsvc%02d" % k, "NodeID": "n%06d" % i, "DesiredState": RUNNING, "Status": {"State": PENDING}, "Spec": spec}


def scheduler(lib, N, S, small_every=0):
    s = swsched.Scheduler(engine=abi.Engine(lib_path=lib))
    for i in range(N):
        s.create_node(node_doc(i, small_every and i % small_every == 0))
    if MOUNTS != "none":
        s.update_volume({"ID": "v0", "Spec": {"Annotations": {"Name": "vol0"}, "Group": "g", "Driver": {"Name": "csi-a"},
                                              "AccessMode": {"Scope": "MULTI_NODE", "Sharing": "ALL"}, "Availability": "ACTIVE"},
                         "VolumeInfo": {"VolumeID": "plug0", "AccessibleTopology": []}})
    for k in range(S):
        s.set_service("gsvc%02d" % k)
        for i in range(N):
            s.create_task(task_doc(k, i))
    return s


def close(s):
    s.close()
    s.e.close()


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--services", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--loop-pairs", type=int, default=2000)
    ap.add_argument("--mounts", choices=["none", "all", "alternate"], default="none")
    a = ap.parse_args()
    global MOUNTS
    MOUNTS = a.mounts
    lib = a.lib or abi.build_library()
    L = abi.load_library(lib)
    has_fit = hasattr(L, "swp_fit_pairs") and (MOUNTS == "none" or hasattr(L, "swp_fit_pairs_volumes"))
    out = {"tool": "bench_preassigned", "nodes": a.nodes, "mounts": MOUNTS, "lib": os.path.relpath(lib, ROOT) if a.lib else "tree", "fit_pairs_exported": hasattr(L, "swp_fit_pairs"),
           "fit_pairs_volumes_exported": hasattr(L, "swp_fit_pairs_volumes"), "cases": []}
    for S in a.services:
        c = {"services": S, "tasks": a.nodes * S}
        best = {}
        for _ in range(a.reps):
            s = scheduler(lib, a.nodes, S)
            ms, dec = timed(s.process_preassigned)
            assert sum(1 for d in dec if d["State"] >= 192) == a.nodes * S, "every task fits in this case"
            best["host_all_fit_ms"] = min(best.get("host_all_fit_ms", 1e18), ms)
            close(s)
            s = scheduler(lib, a.nodes, S, small_every=5)
            ms, dec = timed(s.process_preassigned)
            pend = sum(1 for d in dec if d["State"] < 192)
            best["host_first_ms"] = min(best.get("host_first_ms", 1e18), ms)
            ms, dec = timed(s.process_preassigned)
            assert len(dec) == pend
            best["host_recheck_ms"] = min(best.get("host_recheck_ms", 1e18), ms)
            c["pending_after_first"] = pend
            close(s)
        c.update({k: round(v, 3) for k, v in best.items()})
        c["host_us_per_task"] = round(best["host_all_fit_ms"] * 1e3 / (a.nodes * S), 3)
        if has_fit:   # the engine call alone, against the loop it stands for on a twin engine
            fa, fb = scheduler(lib, a.nodes, S), scheduler(lib, a.nodes, S)
            tmpls = np.concatenate([fa.task_desc(task_doc(k, 0)) for k in range(S)])
            tmplb = np.concatenate([fb.task_desc(task_doc(k, 0)) for k in range(S)])
            pairs = np.array([(fa.node_index("n%06d" % i), k) for k in range(S) for i in range(a.nodes)], dtype=abi.FIT_PAIR_DTYPE)
            fa.e.state_save()
            times = []
            for _ in range(a.reps + 1):
                if MOUNTS == "none":
                    ms, ff = timed(lambda: fa.e.fit_pairs(tmpls, pairs))
                else:
                    ms, (ff, att) = timed(lambda: fa.e.fit_pairs_volumes(tmpls, pairs))
                    assert ((att[:, 0] != abi.NO_VOLUME) == np.array([mounts_of(int(k)) for k in pairs["tmpl"]])).all()
                times.append(ms)
                assert (ff == -1).all()
                fa.e.state_restore()
            c["fit_pairs_ms"] = round(min(times[1:]), 3)   # (the first call warms the arena and the module)
            n = min(a.loop_pairs, len(pairs))
            fb.e.L.swp_choose_volumes.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
            row, n_out, failed = (ctypes.c_uint32 * abi.MAX_MOUNTS)(), ctypes.c_uint32(), ctypes.c_uint32()

            def loop():
                for node, k in pairs[:n]:
                    t = tmplb[k]
                    if fb.e.check_node(t, int(node)) == -1:
                        if int(t["flags"]) >> 8:
                            fb.e._ck(fb.e.L.swp_choose_volumes(fb.e.h, int(t["flags"]) >> 8, int(node), row, ctypes.byref(n_out), ctypes.byref(failed)))
                        fb.e.commit(np.array([(node, t["service"], t["cpu"], t["mem"], t["port_set"], 1)], dtype=abi.PLACEMENT_DTYPE))
            ms, _ = timed(loop)
            c["loop_pairs_timed"] = n
            c["loop_us_per_pair"] = round(ms * 1e3 / n, 2)
            c["loop_ms"] = round(ms * len(pairs) / n, 1)
            c["fit_pairs_speedup_vs_loop"] = round(c["loop_ms"] / c["fit_pairs_ms"], 1)
            close(fa)
            close(fb)
        out["cases"].append(c)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
