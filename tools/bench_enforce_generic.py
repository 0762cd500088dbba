#!/usr/bin/env python3
"""The enforcer sweep on a cluster with generic resources: N nodes x 9 tasks, every node offering 8 named `gpu` values and one Discrete
kind, a third of the tasks holding assignments (one named gpu, every other one of them an fpga unit too). One JSON line.

  host_ms             swp_sched_enforce over the whole request (JSON in, JSON out), best of --reps
  generic_ms          the struct ABI alone: swp_enforce_generic over the same records and lists
  enforce_plain_ms    ... next to swp_enforce over the same records WITHOUT the assignments

--lib PATH runs against another build of libswp.so (an older commit's, for a same-box "before"): a library without
swp_enforce_generic walks the nodes with assignments in the host layer after swp_enforce, and generic_ms is left out.

usage: python tools/bench_enforce_generic.py [--nodes 10000] [--reps 3] [--lib PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from swarmkit_amd import abi, sched as swsched  # noqa: E402

RUNNING, READY = 512, 2
TASKS_PER_NODE, NAMED = 9, 8


def node_doc(i):
    generic = [{"Named": {"Kind": "gpu", "Value": "gpu%d" % q}} for q in range(NAMED)] + [{"Discrete": {"Kind": "fpga", "Value": 4}}]
    return {"ID": "n%06d" % i, "Spec": {"Annotations": {"Name": "node%d" % i, "Labels": {"zone": "z%d" % (i % 4)}}, "Availability": 0},
            "Status": {"State": READY, "Addr": "10.%d.%d.%d" % (i >> 16, (i >> 8) & 255, i & 255)},
            "Description": {"Hostname": "h%d" % i, "Platform": {"Architecture": "amd64", "OS": "linux"},
                            "Resources": {"NanoCPUs": 64 * 10**9, "MemoryBytes": 256 << 30, "Generic": generic}}}


def assignment(i, j):
    """Task j of node i: every third task holds a named gpu; the task with j == 6 of every seventh node one that an earlier task took
    (the node's walk ends there)."""
    if j % 3 != 0:
        return None
    q = j // 3 if not (j == 6 and i % 7 == 0) else 0
    a = [{"Named": {"Kind": "gpu", "Value": "gpu%d" % q}}]
    if j == 3:
        a.append({"Discrete": {"Kind": "fpga", "Value": 1}})
    return a


def task_doc(i, j):
    t = {"ID": "t%06d-%d" % (i, j), "ServiceID": "svc%d" % (j % 3), "NodeID": "n%06d" % i, "DesiredState": RUNNING, "Status": {"State": RUNNING},
         "Spec": {"Resources": {"Reservations": {"NanoCPUs": 10**9, "MemoryBytes": 1 << 30}}}}
    a = assignment(i, j)
    if a is not None:
        t["AssignedGenericResources"] = a
    return t


SERVICES = {"svc0": {"ID": "svc0", "Spec": {"Task": {"Placement": {"Constraints": ["node.labels.zone!=nowhere"]}}}},
            "svc1": {"ID": "svc1", "Spec": {"Task": {"Placement": {"Constraints": ["node.labels.zone!=z3"]}}}},
            "svc2": {"ID": "svc2", "Spec": {"Task": {}}}}


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    lib = a.lib or abi.build_library()
    L = abi.load_library(lib)
    has = hasattr(L, "swp_enforce_generic")
    N = a.nodes
    s = swsched.Scheduler(engine=abi.Engine(lib_path=lib))
    nodes = [node_doc(i) for i in range(N)]
    for nd in nodes:
        s.create_node(nd)
    tbn = {nd["ID"]: [task_doc(i, j) for j in range(TASKS_PER_NODE)] for i, nd in enumerate(nodes)}
    out = {"tool": "bench_enforce_generic", "nodes": N, "tasks": N * TASKS_PER_NODE, "tasks_with_assignments": N * 3, "lib": os.path.relpath(lib, ROOT) if a.lib else "tree",
           "enforce_generic_exported": has}
    times, answer = [], None
    for _ in range(a.reps + 1):
        ms, got = timed(lambda: s.enforce(nodes, tbn, SERVICES))
        times.append(ms)
        assert answer is None or got == answer
        answer = got
    out["host_ms"] = round(min(times[1:]), 3)      # (the first call warms the arena and the module)
    out["host_ms_all"] = [round(t, 3) for t in times[1:]]
    out["rejected"] = sum(len(v) for v in answer.values())
    # the struct ABI on the same request
    e = s.e
    cs = {k: s.constraint_set(v["Spec"]["Task"].get("Placement", {}).get("Constraints", [])) for k, v in SERVICES.items()}
    gpu, fpga = e.intern(abi.SPACE_GENERIC_KIND, "gpu"), e.intern(abi.SPACE_GENERIC_KIND, "fpga")
    nrec = np.zeros(N, dtype=abi.ENF_NODE_DTYPE)
    nrec["node"] = [e.intern(abi.SPACE_NODE_ID, nd["ID"]) for nd in nodes]
    nrec["first_task"] = np.arange(N) * TASKS_PER_NODE
    nrec["n_tasks"] = TASKS_PER_NODE
    nrec["cpu"], nrec["mem"] = 64 * 10**9, 256 << 30
    trec = np.zeros(N * TASKS_PER_NODE, dtype=abi.ENF_TASK_DTYPE)
    trec["cpu"], trec["mem"], trec["flags"] = 10**9, 1 << 30, abi.ENF_RESERVATIONS
    trec["constraint_set"] = np.tile([cs["svc%d" % (j % 3)] for j in range(TASKS_PER_NODE)], N)
    trec["desired_state"] = trec["state"] = RUNNING
    one = [(gpu, 1, q) for q in range(NAMED)] + [(fpga, 0, 4)]
    nres = np.array(one * N, dtype=abi.ENF_RES_DTYPE)
    noff = np.arange(N + 1, dtype=np.uint32) * len(one)
    tres, toff = [], [0]
    for i in range(N):
        for j in range(TASKS_PER_NODE):
            for x in assignment(i, j) or []:
                (ty, spec), = x.items()
                tres.append((gpu, 1, int(spec["Value"][3:])) if ty == "Named" else (fpga, 0, spec["Value"]))
            toff.append(len(tres))
    tres = np.array(tres, dtype=abi.ENF_RES_DTYPE)
    toff = np.array(toff, dtype=np.uint32)
    if has:
        times = []
        for _ in range(a.reps + 1):
            ms, rej = timed(lambda: e.enforce_generic(nrec, trec, noff, nres, toff, tres))
            times.append(ms)
        assert int(rej.sum()) == out["rejected"], "the struct ABI and the host layer reject the same number of tasks"
        out["generic_ms"] = round(min(times[1:]), 3)
    times = []
    for _ in range(a.reps + 1):
        ms, rej = timed(lambda: e.enforce(nrec, trec))
        times.append(ms)
    out["enforce_plain_ms"] = round(min(times[1:]), 3)
    out["rejected_plain"] = int(rej.sum())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
