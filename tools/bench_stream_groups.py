#!/usr/bin/env python3
"""What the streamed tick of task groups (swp_schedule_groups_streamed) gives a caller on the grouped benchmark — cfg3, 1 000 groups of
100 tasks on 10 000 nodes, the groups as bench.py --mode grouped builds them — against the plain swp_schedule_groups call on the same
box in the same run: one JSON line (and --out FILE, e.g. profiles/bench_stream_groups.json). The sibling of tools/bench_stream.py.

Every figure is the wall time of the whole call from the same saved state (swp_state_save / swp_state_restore between calls), in
--rounds rounds (default 3) of --reps calls each; per round the median, over the rounds min / median / max.

  (a) plain          swp_schedule_groups on the tree's library — and on --parent PATH (the parent commit's libswp.so, built as
                     tools/README.md says for gpu_ab.sh), the order alternating from round to round: the plain path must not have
                     become slower (beyond the spread the parent's rounds show among themselves)
  (b) streamed       swp_schedule_groups_streamed with a sink that does nothing, default step: time to return, time to the first sink
                     call, calls
  (c) step           the same with SWP_STREAM_GROUP_TASKS = 128, 1024, 8192
  (d) kernel         the tick's two launches between two events (SWP_DBG=16: the engine prints them), plain instance against streamed
                     instance at each step of (c), --reps runs each, alternating: the publish commands must not lengthen the machine's chain

usage: python tools/bench_stream_groups.py [--parent PATH] [--tasks 100000] [--nodes 10000] [--rounds 3] [--reps 5] [--out FILE]"""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from swarmkit_amd import abi, synth, sched as swsched  # noqa: E402
from swarmkit_amd import host as swhost  # noqa: E402

STEPS = (128, 1024, 8192)


class Side:
    """One library: an engine with the workload loaded and its state saved."""

    def __init__(self, name, lib, wl):
        self.name = name
        self.s = swsched.Scheduler(engine=abi.Engine(lib_path=lib))
        descs = np.ascontiguousarray(swhost.load_workload(self.s, wl), dtype=abi.TASK_DTYPE)
        self.groups = np.ascontiguousarray(descs[:wl.S])   # (round-robin order: the first S tasks are one of each service)
        self.sizes = np.bincount(np.array([wl.task_service(j) for j in range(wl.T)]), minlength=wl.S).astype(np.uint32)
        self.e = self.s.e
        self.out = np.empty(wl.T, dtype=np.int32)
        self.hist = np.zeros((wl.S, abi.NFILTERS), dtype=np.uint32)
        self.e.state_save()
        self.streams = hasattr(self.e.L, "swp_schedule_groups_streamed")
        self.first = self.calls = 0

        def cb(_ctx, _first, _count, _nodes):
            if not self.calls:
                self.first = time.perf_counter()
            self.calls += 1
            return 0
        self.cb = abi.PREFIX_SINK(cb)
        self.plain()   # warm: modules, pools, the pinned blocks
        self.want = self.out.copy()
        if self.streams:
            self.streamed(0)
            assert (self.out == self.want).all(), "the streamed tick and the plain tick disagree"

    def plain(self):
        t = time.perf_counter()
        self.e._ck(self.e.L.swp_schedule_groups(self.e.h, self.groups.ctypes.data, self.sizes.ctypes.data, len(self.groups), self.out.ctypes.data, self.hist.ctypes.data))
        dt = (time.perf_counter() - t) * 1e3
        self.e.state_restore()
        return dt

    def streamed(self, min_tasks):
        self.calls = 0
        t = time.perf_counter()
        self.e._ck(self.e.L.swp_schedule_groups_streamed(self.e.h, self.groups.ctypes.data, self.sizes.ctypes.data, len(self.groups), self.out.ctypes.data, self.hist.ctypes.data,
                                                         None, self.cb, None, min_tasks))
        t1 = time.perf_counter()
        self.e.state_restore()
        return (t1 - t) * 1e3, (self.first - t) * 1e3, self.calls


def summary(per_round):
    return {"rounds": [round(x, 3) for x in per_round], "min": round(min(per_round), 3), "median": round(statistics.median(per_round), 3), "max": round(max(per_round), 3)}


def kernel_ms(fn, pattern):
    """fn() with SWP_DBG=16 and the process's stderr in a file: the engine's own event pair around the tick's launches"""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        os.environ["SWP_DBG"] = "16"
        try:
            fn()
        finally:
            os.environ.pop("SWP_DBG", None)
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        m = re.search(pattern, f.read().decode(errors="replace"))
    return float(m.group(1)) if m else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--tasks", type=int, default=100_000)
    ap.add_argument("--nodes", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-tasks", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for k in ("SWP_STREAM_GROUP_TASKS", "SWP_DBG"):
        os.environ.pop(k, None)
    wl = synth.Workload("cfg3", T=a.tasks, N=a.nodes)
    sides = []
    if a.parent:
        sides.append(Side("parent", os.path.abspath(a.parent), wl))
    sides.append(Side("tree", abi.build_library(), wl))
    tree = sides[-1]
    if a.parent:
        assert (sides[0].want == tree.want).all(), "the two libraries place the tick differently"
    plain = {s.name: [] for s in sides}
    ret, first, calls = [], [], []
    step = {k: {"ret": [], "first": [], "calls": []} for k in STEPS}
    for r in range(a.rounds):
        for s in (sides if r % 2 == 0 else sides[::-1]):
            plain[s.name].append(statistics.median(s.plain() for _ in range(a.reps)))
        got = [tree.streamed(a.min_tasks) for _ in range(a.reps)]
        ret.append(statistics.median(g[0] for g in got))
        first.append(statistics.median(g[1] for g in got))
        calls.append(got[-1][2])
        for k in (STEPS if r % 2 == 0 else STEPS[::-1]):
            os.environ["SWP_STREAM_GROUP_TASKS"] = str(k)
            got = [tree.streamed(a.min_tasks) for _ in range(a.reps)]
            step[k]["ret"].append(statistics.median(g[0] for g in got))
            step[k]["first"].append(statistics.median(g[1] for g in got))
            step[k]["calls"].append(got[-1][2])
        os.environ.pop("SWP_STREAM_GROUP_TASKS", None)
    # (d) the kernel alone
    k_plain, k_streamed = [], {k: [] for k in STEPS}
    for _ in range(a.reps):
        k_plain.append(kernel_ms(tree.plain, r"k_groups2 ([0-9.]+) ms"))
        for k in STEPS:
            os.environ["SWP_STREAM_GROUP_TASKS"] = str(k)
            k_streamed[k].append(kernel_ms(lambda: tree.streamed(a.min_tasks), r"k_groups2s ([0-9.]+) ms"))
        os.environ.pop("SWP_STREAM_GROUP_TASKS", None)
    out = {"tool": "bench_stream_groups", "workload": "cfg3", "tasks": a.tasks, "nodes": a.nodes, "groups": int(wl.S), "rounds": a.rounds, "reps": a.reps, "min_tasks": a.min_tasks,
           "placed": int((tree.want >= 0).sum()),
           "a_plain_ms": {k: summary(v) for k, v in plain.items()},
           "b_streamed": {"step": 1024, "return_ms": summary(ret), "first_sink_call_ms": summary(first), "sink_calls": calls},
           "c_step_sweep": {str(k): {"return_ms": summary(v["ret"]), "first_sink_call_ms": summary(v["first"]), "sink_calls": v["calls"]} for k, v in step.items()},
           "d_kernel_ms": {"plain_k_groups2": summary(k_plain), "streamed_k_groups2s": {str(k): summary(v) for k, v in k_streamed.items()}}}
    out["d_kernel_ms"]["plain_spread_ms"] = round(max(k_plain) - min(k_plain), 3)
    out["d_kernel_ms"]["streamed_1024_minus_plain_median_ms"] = round(statistics.median(k_streamed[1024]) - statistics.median(k_plain), 3)
    if a.parent:
        p, t = out["a_plain_ms"]["parent"], out["a_plain_ms"]["tree"]
        out["plain_parent_spread_ms"] = round(p["max"] - p["min"], 3)
        out["plain_tree_minus_parent_ms"] = round(t["median"] - p["median"], 3)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
