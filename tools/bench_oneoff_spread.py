#!/usr/bin/env python3
"""What keeping one-off tasks with spread preferences in the tick's batch (SWP_SCHED_ONEOFF_SPREAD=1, csrc/swp_sched.cpp; the batch's
spread segments, csrc/swp_scan_spread.hpp) gives a caller, against the host layer's default — the run of one-off tasks cut at every such
task, each sent through swp_schedule_groups as a group of one — on the same box in the same run: one JSON line (and --out FILE, e.g.
profiles/oneoff_spread.json).

  (a) tick        swp_sched_tick over --tasks one-off tasks of --services services, every one with `spread=node.labels.zone`, on --nodes
                  nodes: the knob off (today's path, the yardstick), then on; --runs fresh schedulers each, wall time of the tick alone,
                  min / median / max and the spread of the runs. Both sides must decide every task alike.
  (b) engine      the knob-on tick's device pass alone: the events around the spread segment (SWP_CFG_PROFILE: swp_stats ms_scan)
                  and around the whole batch (ms_total), per task.
  (c) tree price  the same descriptors through swp_schedule_batch with and without their preferences, engine events per task — at
                  the shape of (a), where tasks without preferences go to the block resolver, and at --scan-shape (few services,
                  more tasks than nodes), where the engine hands them to the scan resolver (k_scan / k_scanb): the counters say
                  which resolver took how many.

  --pool        the COMPACT form instead of (a) - (c) (csrc/swp_scan_spread.hpp, k_scan_spread<.., true>: a nodeSet beyond 4 096 slots):
                  --pool-nodes nodes (default 10 000) of which every --pool-every-th (10) carries pool=a, spread over --zones zones;
                  the tasks are constrained to the pool. The tick with the knob off (the parent's behaviour: the batch is refused
                  there, the host layer splits) and on, --runs fresh schedulers each; then the PLAIN instance on a cluster made of
                  just the pool's nodes, knob on: the difference is the cost of compaction (probe, gather, base sums, indirection).
                  e.g. --pool --out profiles/oneoff_spread_compact.json
  --riders      with --pool: after every --riders-every (50) pooled spread tasks come --riders-count (10) UNCONSTRAINED plain one-off
                  tasks. The one spread segment of the tick then has the whole nodeSet as its union; the preparation cuts it
                  (csrc/swp_scan_spread.hpp k_spread_cut) into a spread segment per run with a stretch of the block resolver per gap.
                  Knob off (what the parent commit does with this tick, knob on or off) against knob on, --runs each; the
                  preparation's share — first probe, cut, second probe — from the engine's own SWP_DEBUG_PREPARE line.
                  e.g. --pool --riders --out profiles/oneoff_spread_cut.json

  --wide        the WIDE form instead of (a) - (c) (csrc/swp_scan_spread.hpp k_scan_spread_wide, SWP_SPREAD_WIDE=1): --wide-nodes nodes
                  (default 10 000) over --zones zones, --tasks UNCONSTRAINED one-off tasks with `spread=node.labels.zone` — each task's own
                  class row is the whole nodeSet. SWP_SCHED_ONEOFF_SPREAD=1 on both sides; SWP_SPREAD_WIDE unset (what the parent commit
                  does with this tick: the batch is refused at its preparation, then a group call per task — the baseline) against
                  SWP_SPREAD_WIDE=1, --runs fresh schedulers each, alternating. Both sides must decide every task alike.
                  e.g. --wide --out profiles/oneoff_spread_wide.json

usage: python tools/bench_oneoff_spread.py [--tasks 20000] [--services 200] [--nodes 1000] [--zones 5] [--runs 3] [--out FILE]
       python tools/bench_oneoff_spread.py --pool [--pool-nodes 10000] [--pool-every 10] [--tasks 20000] [--services 200] [--runs 3] [--out FILE]
       python tools/bench_oneoff_spread.py --pool --riders [--riders-every 50] [--riders-count 10] [--runs 3] [--out FILE]
       python tools/bench_oneoff_spread.py --wide [--wide-nodes 10000] [--tasks 20000] [--services 200] [--runs 3] [--out FILE]"""
import argparse
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from swarmkit_amd import abi  # noqa: E402
from swarmkit_amd import host as swhost  # noqa: E402

READY, RUNNING, PENDING, ASSIGNED = 2, 512, 64, 192
KNOB = "SWP_SCHED_ONEOFF_SPREAD"
WIDE = "SWP_SPREAD_WIDE"   # (read once, when the engine is created)


def node_doc(i, zones):
    return {"ID": "n%05d" % i, "Status": {"State": READY}, "Spec": {"Annotations": {"Labels": {"zone": "z%d" % (i % zones)}}},
            "Description": {"Resources": {"NanoCPUs": 64 * 10**9, "MemoryBytes": 256 << 30}}}


def task_doc(j, services, prefs=True):
    spec = {"Resources": {"Reservations": {"NanoCPUs": 10**8, "MemoryBytes": 64 << 20}}}
    if prefs:
        spec["Placement"] = {"Preferences": [{"Spread": {"SpreadDescriptor": "node.labels.zone"}}]}
    return {"ID": "t%06d" % j, "ServiceID": "svc%03d" % (j % services), "DesiredState": RUNNING, "Status": {"State": PENDING}, "Spec": spec}


def loaded(a, knob, profile=False, tasks=True):
    if knob:
        os.environ[KNOB] = "1"
    else:
        os.environ.pop(KNOB, None)
    s = swhost.HostScheduler(profile=profile)
    for i in range(a.nodes):
        s.create_node(node_doc(i, a.zones))
    for k in range(a.services):
        s.set_service("svc%03d" % k)
    if tasks:
        for j in range(a.tasks):
            s.create_task(task_doc(j, a.services))
    return s


def one_tick(a, knob, profile=False):
    s = loaded(a, knob, profile)
    t = time.perf_counter()
    d = s.tick()
    ms = (time.perf_counter() - t) * 1e3
    st = s.e.stats()
    return ms, {x["ID"]: x["NodeID"] for x in d}, st


def pool_node_doc(i, zones, every):
    labels = {"zone": "z%d" % (i // every % zones)}
    if i % every == 0:
        labels["pool"] = "a"
    return {"ID": "n%05d" % i, "Status": {"State": READY}, "Spec": {"Annotations": {"Labels": labels}},
            "Description": {"Resources": {"NanoCPUs": 64 * 10**9, "MemoryBytes": 256 << 30}}}


def rider_doc(j, services):
    return {"ID": "t%06d" % j, "ServiceID": "svc%03d" % (j % services), "DesiredState": RUNNING, "Status": {"State": PENDING},
            "Spec": {"Resources": {"Reservations": {"NanoCPUs": 10**8, "MemoryBytes": 64 << 20}}}}


def pool_tick(a, knob, only_pool, profile=False):
    """one tick of --tasks pooled spread tasks; only_pool: the cluster is just the pool's nodes (the plain instance);
    --riders: unconstrained plain tasks between runs of them (ids in creation order)"""
    if knob:
        os.environ[KNOB] = "1"
    else:
        os.environ.pop(KNOB, None)
    s = swhost.HostScheduler(profile=profile)
    for i in range(a.pool_nodes):
        if not only_pool or i % a.pool_every == 0:
            s.create_node(pool_node_doc(i, a.zones, a.pool_every))
    for k in range(a.services):
        s.set_service("svc%03d" % k)
    at = 0
    for j in range(a.tasks):
        t = task_doc(at, a.services)
        t["Spec"]["Placement"]["Constraints"] = ["node.labels.pool==a"]
        s.create_task(t)
        at += 1
        if getattr(a, "riders", False) and (j + 1) % a.riders_every == 0 and j + 1 < a.tasks:
            for _ in range(a.riders_count):
                s.create_task(rider_doc(at, a.services))
                at += 1
    t0 = time.perf_counter()
    d = s.tick()
    ms = (time.perf_counter() - t0) * 1e3
    return ms, {x["ID"]: x["NodeID"] for x in d}, s.e.stats()


def prepare_lines(a):
    """one more knob-on tick with SWP_DEBUG_PREPARE set and the process's stderr in a file: the engine's own lines about the preparation"""
    path = (a.out or "/tmp/bench_oneoff_spread") + ".stderr"
    sys.stderr.flush()
    keep, fd = os.dup(2), os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    os.dup2(fd, 2)
    os.environ["SWP_DEBUG_PREPARE"] = "1"
    try:
        pool_tick(a, True, False)
    finally:
        os.environ.pop("SWP_DEBUG_PREPARE", None)
        os.dup2(keep, 2)
        os.close(fd)
        os.close(keep)
    text = open(path).read()
    os.remove(path)
    out = {}
    m = re.search(r"spread cut: (\d+) of (\d+) segments too wide, limit (\d+) nodes: (\d+) segments now; first probe ([\d.]+) ms, cut ([\d.]+) ms, second probe ([\d.]+) ms", text)
    if m:
        out = {"segments_too_wide": int(m.group(1)), "segments_before": int(m.group(2)), "limit_nodes": int(m.group(3)), "segments_after": int(m.group(4)),
               "first_probe_ms": float(m.group(5)), "cut_ms": float(m.group(6)), "second_probe_ms": float(m.group(7))}
    m = re.search(r"swp_batch_prepare (\d+) tasks: build ([\d.]+) ms, upload ([\d.]+) ms", text)
    if m:
        out.update(prepare_build_ms=float(m.group(2)), prepare_upload_and_probes_ms=float(m.group(3)))
    return out


def riders_main(a):
    os.environ["SWP_HOST"] = "cxx"
    one_tick(argparse.Namespace(nodes=64, zones=a.zones, services=4, tasks=64), True)   # warm: modules, pools
    n_runs = (a.tasks + a.riders_every - 1) // a.riders_every
    off, on, want, st_on = [], [], None, None
    for r in range(a.runs):
        for knob in ((False, True) if r % 2 == 0 else (True, False)):
            ms, dec, st = pool_tick(a, knob, False)
            (on if knob else off).append(ms)
            if want is None:
                want = dec
            assert dec == want, "the two paths decide the tick differently"
            if knob:
                assert st["scan_tasks"] >= a.tasks and st["scan_launches"] >= n_runs, st
                st_on = st
    ms, _, st = pool_tick(a, True, False, profile=True)
    eng = {"tick_ms_with_profile": round(ms, 3), "spread_segments_ms": round(st["ms_scan"], 3), "batch_ms_total": round(st["ms_total"], 3)}
    out = {"tool": "bench_oneoff_spread --pool --riders", "spread_tasks": a.tasks, "riders": len(want) - a.tasks, "riders_every": a.riders_every, "riders_count": a.riders_count,
           "services": a.services, "nodes": a.pool_nodes, "pool_nodes": len(range(0, a.pool_nodes, a.pool_every)), "zones": a.zones, "runs": a.runs,
           "placed": sum(1 for v in want.values() if v), "spread_runs": n_runs,
           "knob_on_counters": {k: st_on[k] for k in ("batches", "scan_launches", "scan_tasks", "resolve_launches")},
           "tick_ms": {"knob_off_parent_path": summary(off), "knob_on_cut": summary(on), "off_over_on_median": round(statistics.median(off) / statistics.median(on), 2)},
           "engine_knob_on": eng, "preparation_knob_on": prepare_lines(a)}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


def pool_main(a):
    if a.riders:
        return riders_main(a)
    os.environ["SWP_HOST"] = "cxx"
    one_tick(argparse.Namespace(nodes=64, zones=a.zones, services=4, tasks=64), True)   # warm: modules, pools
    off, on, plain, want = [], [], [], None
    for r in range(a.runs):
        for knob in ((False, True) if r % 2 == 0 else (True, False)):
            ms, dec, st = pool_tick(a, knob, False)
            (on if knob else off).append(ms)
            if want is None:
                want = dec
            assert dec == want, "the two paths decide the tick differently"
            if knob:
                assert st["scan_tasks"] == a.tasks and st["scan_launches"] == 1, st
        ms, dec, st = pool_tick(a, True, True)
        assert dec == want and st["scan_tasks"] == a.tasks, "the pool alone decides the tick differently"
        plain.append(ms)
    eng = {}
    for name, only_pool in (("compact", False), ("plain_pool_alone", True)):
        ms, _, st = pool_tick(a, True, only_pool, profile=True)
        eng[name] = {"tick_ms_with_profile": round(ms, 3), "segment_ms": round(st["ms_scan"], 3), "batch_ms_total": round(st["ms_total"], 3),
                     "segment_us_per_task": round(st["ms_scan"] * 1e3 / a.tasks, 3)}
    out = {"tool": "bench_oneoff_spread --pool", "tasks": a.tasks, "services": a.services, "nodes": a.pool_nodes, "pool_nodes": len(range(0, a.pool_nodes, a.pool_every)),
           "zones": a.zones, "runs": a.runs, "placed": sum(1 for v in want.values() if v),
           "tick_ms": {"knob_off_parent_path": summary(off), "knob_on_compact": summary(on), "knob_on_plain_pool_alone": summary(plain),
                       "off_over_on_median": round(statistics.median(off) / statistics.median(on), 2),
                       "compact_over_plain_median": round(statistics.median(on) / statistics.median(plain), 3)},
           "engine_knob_on": eng}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


def wide_main(a):
    os.environ["SWP_HOST"] = "cxx"
    os.environ.pop(WIDE, None)
    one_tick(argparse.Namespace(nodes=64, zones=a.zones, services=4, tasks=64), True)   # warm: modules, pools
    shape = argparse.Namespace(nodes=a.wide_nodes, zones=a.zones, services=a.services, tasks=a.tasks)

    def side(wide, profile=False):
        if wide:
            os.environ[WIDE] = "1"
        else:
            os.environ.pop(WIDE, None)
        try:
            return one_tick(shape, True, profile)
        finally:
            os.environ.pop(WIDE, None)

    off, on, want, st_on, st_off = [], [], None, None, None
    for r in range(a.runs):
        for wide in ((False, True) if r % 2 == 0 else (True, False)):
            ms, dec, st = side(wide)
            (on if wide else off).append(ms)
            if want is None:
                want = dec
            assert dec == want, "the two sides decide the tick differently"
            if wide:
                assert st["scan_tasks"] == a.tasks and st["scan_launches"] == 1, st
                st_on = st
            else:
                assert st["scan_tasks"] == 0, st   # (refused at the preparation: no spread segment ran)
                st_off = st
    ms, _, st = side(True, profile=True)
    eng = {"tick_ms_with_profile": round(ms, 3), "segment_ms": round(st["ms_scan"], 3), "batch_ms_total": round(st["ms_total"], 3),
           "segment_us_per_task": round(st["ms_scan"] * 1e3 / a.tasks, 3)}
    out = {"tool": "bench_oneoff_spread --wide", "tasks": a.tasks, "services": a.services, "nodes": a.wide_nodes, "zones": a.zones, "runs": a.runs,
           "placed": sum(1 for v in want.values() if v),
           "counters": {"wide_unset_parent_path": {k: st_off[k] for k in ("batches", "scan_launches", "scan_tasks")}, "wide_on": {k: st_on[k] for k in ("batches", "scan_launches", "scan_tasks")}},
           "tick_ms": {"wide_unset_parent_path": summary(off), "wide_on": summary(on), "unset_over_on_median": round(statistics.median(off) / statistics.median(on), 2)},
           "engine_wide_on": eng}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


def summary(v):
    return {"runs": [round(x, 3) for x in v], "min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3), "spread": round(max(v) - min(v), 3)}


def batch_events(n_nodes, zones, services, n_tasks, prefs):
    """one swp_schedule_batch over the descriptors on a fresh engine with SWP_CFG_PROFILE: the engine's own events"""
    os.environ.pop(KNOB, None)
    s = swhost.HostScheduler(profile=True)
    for i in range(n_nodes):
        s.create_node(node_doc(i, zones))
    for k in range(services):
        s.set_service("svc%03d" % k)
    per = np.concatenate([s.task_desc(task_doc(k, services, prefs)) for k in range(services)])
    descs = np.ascontiguousarray(per[np.arange(n_tasks) % services], dtype=abi.TASK_DTYPE)
    out, _ = s.e.schedule_batch(descs)
    st = s.e.stats()
    return {"placed": int((out >= 0).sum()), "ms_total": round(st["ms_total"], 3), "ms_scan": round(st["ms_scan"], 3), "ms_resolve": round(st["ms_resolve"], 3),
            "scan_tasks": st["scan_tasks"], "scan_batched_tasks": st["scan_batched_tasks"], "scan_launches": st["scan_launches"], "resolve_launches": st["resolve_launches"],
            "us_per_task": round(st["ms_resolve"] * 1e3 / n_tasks, 3)}, out   # (ms_resolve: the resolvers' whole phase, the scan resolver's share — ms_scan — included)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tasks", type=int, default=20_000)
    ap.add_argument("--services", type=int, default=200)
    ap.add_argument("--nodes", type=int, default=1000)
    ap.add_argument("--zones", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--scan-shape", default="10,500,20000", help="services,nodes,tasks of (c)'s second shape")
    ap.add_argument("--out", default=None)
    ap.add_argument("--pool", action="store_true", help="the compact form: a labelled pool of a cluster beyond 4 096 nodes")
    ap.add_argument("--pool-nodes", type=int, default=10_000)
    ap.add_argument("--pool-every", type=int, default=10)
    ap.add_argument("--riders", action="store_true", help="with --pool: unconstrained plain one-off tasks between runs of the pooled spread tasks (the segment is cut)")
    ap.add_argument("--riders-every", type=int, default=50)
    ap.add_argument("--riders-count", type=int, default=10)
    ap.add_argument("--wide", action="store_true", help="the wide form: unconstrained spread tasks on a cluster beyond 4 096 nodes, SWP_SPREAD_WIDE=1 against unset")
    ap.add_argument("--wide-nodes", type=int, default=10_000)
    a = ap.parse_args()
    if a.wide:
        return wide_main(a)
    if a.pool:
        return pool_main(a)
    os.environ["SWP_HOST"] = "cxx"
    one_tick(argparse.Namespace(nodes=64, zones=a.zones, services=4, tasks=64), True)   # warm: modules, pools
    off, on, want = [], [], None
    for r in range(a.runs):
        for knob in ((False, True) if r % 2 == 0 else (True, False)):
            ms, dec, st = one_tick(a, knob)
            (on if knob else off).append(ms)
            if want is None:
                want = dec
            assert dec == want, "the two paths decide the tick differently"
            if knob:
                assert st["scan_tasks"] == a.tasks, st
    ms, _, st = one_tick(a, True, profile=True)
    engine = {"tick_ms_with_profile": round(ms, 3), "segment_ms": round(st["ms_scan"], 3), "batch_ms_total": round(st["ms_total"], 3),
              "segment_us_per_task": round(st["ms_scan"] * 1e3 / a.tasks, 3), "scan_launches": st["scan_launches"], "scan_tasks": st["scan_tasks"]}
    tree = {}
    sv, nn, tt = (int(x) for x in a.scan_shape.split(","))
    for name, (services, nodes, tasks) in (("tick_shape", (a.services, a.nodes, a.tasks)), ("scan_shape", (sv, nn, tt))):
        with_p, out_p = batch_events(nodes, a.zones, services, tasks, True)
        without, out_n = batch_events(nodes, a.zones, services, tasks, False)
        tree[name] = {"services": services, "nodes": nodes, "tasks": tasks, "with_preferences": with_p, "without_preferences": without}
    out = {"tool": "bench_oneoff_spread", "tasks": a.tasks, "services": a.services, "nodes": a.nodes, "zones": a.zones, "runs": a.runs,
           "placed": sum(1 for v in want.values() if v),
           "a_tick_ms": {"knob_off_parent_path": summary(off), "knob_on": summary(on), "off_over_on_median": round(statistics.median(off) / statistics.median(on), 2)},
           "b_engine_knob_on": engine, "c_tree_price": tree}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
