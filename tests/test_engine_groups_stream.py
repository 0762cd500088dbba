"""GPU: the streamed tick of task groups (include/swp.h swp_schedule_groups_streamed) — the streamed instance of the group kernel
(k_groups2s) publishes the placements of the groups decided so far to host-visible memory from inside its one long launch, and the
caller's sink receives them, folded into the node mirror, while later groups are decided.

Through the struct ABI. The judges: a plain swp_schedule_groups / swp_schedule_groups_volumes call on a twin engine (placements,
Explain counters, attachments, every node row, generic and per-service counts), and the oracle (tests/orc.py), which gets the same
groups one per tick — a tick decides its groups one after the other against the state the earlier ones left, so that is the same
sequence; which of a group's tasks goes where inside the group is the caller's order, so a group is compared as the multiset of its nodes
and its Err string. For every case the ranges the sink saw are contiguous, ascending, end at group boundaries, cover the tick once and
respect min_tasks. The twin's and the oracle's answers for a tick are computed once and shared."""
import collections
import ctypes as C
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import kat_volumes as kv
import orc
import scenarios as sc
from swarmkit_amd import abi, synth
from swarmkit_amd import host as swhost

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    monkeypatch.setenv("SWP_HOST", "cxx")   # (the Python twin of the host layer knows no volumes)
    monkeypatch.delenv("SWP_STREAM_GROUP_TASKS", raising=False)


class Tick:
    """Node, volume and service documents and the groups of one tick — (a task document without ID, tasks) in order: the same into the
    oracle and into an engine. Every group of a service carries the same SpecVersion (one device call does not mix a service's versions); two groups of
    one service are then two calls of scheduleTaskGroup for the oracle because they reach it in different ticks."""

    def __init__(self, key, nodes, services, groups, volumes=()):
        self.key, self.nodes, self.services, self.groups, self.volumes = key, list(nodes), list(services), list(groups), list(volumes)
        self.sizes = np.array([k for _, k in self.groups], dtype=np.uint32)
        self.ends = np.cumsum(self.sizes)
        self.total = int(self.sizes.sum())


_oracle, _plain = {}, {}


def oracle_of(t):
    """Per group: (Counter of node ids, tasks left over, their Err), the groups one per tick; computed once per Tick."""
    if t.key not in _oracle:
        o = orc.Oracle()
        for d in t.nodes:
            o.create_node(d)
        for v in t.volumes:
            o.update_volume(v)
        for s in t.services:
            o.set_service(s)
        res = []
        for g, (doc, k) in enumerate(t.groups):
            docs = {"g%04d-%05d" % (g, i): dict(doc, ID="g%04d-%05d" % (g, i)) for i in range(k)}
            for d in docs.values():
                o.create_task(d)
            placed, errs, n = collections.Counter(), set(), 0
            for d in o.tick():
                if d["ID"] not in docs:
                    # a task an earlier group left over is tried again with every tick (the engine's tick has no such retry). It finds
                    # nothing: no node's residuals, counts or ports ever get better while groups are only placed.
                    assert not (d["State"] >= orc.ASSIGNED and d["NodeID"]), d
                    continue
                n += 1
                if d["State"] >= orc.ASSIGNED and d["NodeID"]:
                    placed[d["NodeID"]] += 1
                else:
                    errs.add(d["Err"])
            assert n == k and len(errs) <= 1
            res.append((placed, k - sum(placed.values()), errs.pop() if errs else None))
        _oracle[t.key] = res
    return _oracle[t.key]


def engine_of(t, **engine_kw):
    """(host scheduler, one descriptor per group): the cluster loaded, the groups' documents translated."""
    s = swhost.HostScheduler(**engine_kw)
    for d in t.nodes:
        s.create_node(d)
    for v in t.volumes:
        s.update_volume(v)
    for sid in t.services:
        s.set_service(sid)
    seen, descs = {}, np.zeros(len(t.groups), dtype=abi.TASK_DTYPE)
    for g, (doc, _) in enumerate(t.groups):
        key = repr(sorted((a, repr(b)) for a, b in doc.items()))
        if key not in seen:
            seen[key] = s.task_desc(dict(doc, ID="x"))[0]
        descs[g] = seen[key]
    return s, descs


def all_rows(s, n):
    return s.e.node_get_many(np.arange(n, dtype=np.uint32)).tobytes() if n else b""


def counts_of(s, t, descs, kinds=()):
    """what a node row does not hold: the per-service counts of the tick's services and the generic counts of `kinds`, for every node"""
    N = len(t.nodes)
    svcs = sorted(set(int(x) for x in descs["service"]))
    return ([[s.e.node_get_svc_count(n, v) for v in svcs] for n in range(N)],
            [[s.e.node_get_generic(n, s.e.intern(abi.SPACE_GENERIC_KIND, k)) for k in kinds] for n in range(N)])


def groups_volumes(e, descs, sizes):
    """swp_schedule_groups_volumes through the raw export (the binding has no method for it)"""
    total = int(sizes.sum())
    out = np.empty(total, dtype=np.int32)
    hist = np.zeros((len(descs), abi.NFILTERS), dtype=np.uint32)
    att = np.full((total, abi.MAX_MOUNTS), abi.NO_VOLUME, dtype=np.uint32)
    fn = e.L.swp_schedule_groups_volumes
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    fn.restype = C.c_int
    e._ck(fn(e.h, descs.ctypes.data, sizes.ctypes.data, len(descs), out.ctypes.data, hist.ctypes.data, att.ctypes.data))
    return out, hist, att


def plain_of(t, kinds=(), volumes=False):
    """The plain call on a twin engine, once per Tick."""
    if t.key not in _plain:
        s, descs = engine_of(t)
        if volumes:
            out, hist, att = groups_volumes(s.e, descs, t.sizes)
        else:
            (out, hist), att = s.e.schedule_groups(descs, t.sizes), None
        _plain[t.key] = dict(out=out, hist=hist, att=att, rows=all_rows(s, len(t.nodes)), counts=counts_of(s, t, descs, kinds), stats=s.e.stats(), s=s)
    return _plain[t.key]


def run_streamed(t, min_tasks=0, inside=None, want_att=False, kinds=()):
    s, descs = engine_of(t)
    calls = []

    def sink(first, nodes):
        calls.append((first, nodes.copy()))
        if inside:
            return inside(s, descs, calls)
    res = s.e.schedule_groups_streamed(descs, t.sizes, sink, min_tasks, want_att=want_att)
    return dict(out=res[0], hist=res[1], att=res[2] if want_att else None, rows=all_rows(s, len(t.nodes)), counts=counts_of(s, t, descs, kinds), stats=s.e.stats(),
                calls=calls, s=s, descs=descs)


def check_ranges(t, calls, min_tasks):
    pos, ends = 0, set(int(x) for x in t.ends)
    for first, nodes in calls:
        assert first == pos and len(nodes) > 0, (first, pos)
        pos += len(nodes)
        assert pos in ends, pos                       # a range ends at a group boundary
    assert pos == t.total
    assert all(len(n) >= max(min_tasks, 1) for _, n in calls[:-1]), [len(n) for _, n in calls]


def check_oracle(t, s, out, hist):
    off = 0
    for g, (want, k) in enumerate(zip(oracle_of(t), t.sizes)):
        placed, left, err = want
        nodes = out[off:off + k]
        off += int(k)
        got = collections.Counter(s.idx_to_id[int(n)] for n in nodes if n >= 0)
        assert got == placed and int((nodes < 0).sum()) == left, (g, got, placed, left)
        if left:
            ex = s.explain(hist[g])
            assert err == ("no suitable node (" + ex + ")" if ex else "no suitable node"), (g, err, ex)


def check_all(t, st, plain, min_tasks=0):
    """What every case is judged by."""
    check_ranges(t, st["calls"], min_tasks)
    seen = np.concatenate([n for _, n in st["calls"]]) if st["calls"] else np.zeros(0, dtype=np.int32)
    assert (seen == plain["out"]).all() and (st["out"] == plain["out"]).all()       # every range held the final answer
    assert (st["hist"] == plain["hist"]).all()
    assert st["rows"] == plain["rows"] and st["counts"] == plain["counts"]
    for k in ("batches", "tasks", "placed", "infeasible"):
        assert st["stats"][k] == plain["stats"][k], k
    check_oracle(t, st["s"], st["out"], st["hist"])


def host_marks(sizes, step):
    """The rule of swp_rounds.hpp group_marks, written again from its statement."""
    out, since, end = [], 0, 0
    for g, k in enumerate(sizes):
        since += int(k)
        end += int(k)
        if since >= step or g == len(sizes) - 1:
            out.append(end)
            since = 0
    return out


def node_doc(i, labels=None, generic=None, cpu=8, mem_gb=16):
    res = {"NanoCPUs": cpu * 10**9, "MemoryBytes": mem_gb << 30}
    if generic:
        res["Generic"] = generic
    return sc.node("n%04d" % i, Spec={"Annotations": {"Labels": labels or {}}}, Description={"Resources": res})


def group_doc(svc, version, **spec):
    return sc.pending("x", svc, version, Spec=spec) if spec else sc.pending("x", svc, version)


# ---- the ticks ----
def cycle_tick():
    """40 groups with sizes cycling 1, 63, 64, 65, 100 on 150 nodes; neighbours sometimes of one service (nothing evaluated ahead)"""
    nodes = [node_doc(i, {"az": "az%d" % (i % 3)}, cpu=4 + i % 3, mem_gb=8 + 4 * (i % 4)) for i in range(150)]
    svcs = ["svc%d" % k for k in range(12)]
    groups = []
    for g in range(40):
        spec = {"Resources": {"Reservations": {"NanoCPUs": (1 + g % 3) * 10**8, "MemoryBytes": (64 + 32 * (g % 4)) << 20}}}
        if g % 4 == 1:
            spec["Placement"] = {"Preferences": [{"Spread": {"SpreadDescriptor": "node.labels.az"}}]}
        groups.append((group_doc(svcs[(g - (g % 7 == 3)) % 12], 1, **spec), [1, 63, 64, 65, 100][g % 5]))
    return Tick("cycle 40 groups x 150 nodes", nodes, svcs, groups)


# 1
def test_ranges_at_every_group(monkeypatch):
    monkeypatch.setenv("SWP_STREAM_GROUP_TASKS", "1")
    t = cycle_tick()
    st = run_streamed(t, 0)
    assert [(f, len(n)) for f, n in st["calls"]] == [(int(e - k), int(k)) for e, k in zip(t.ends, t.sizes)]   # exactly 40 calls: the group bounds
    assert len(st["calls"]) == 40
    check_all(t, st, plain_of(t))
    again = run_streamed(t, 0)
    assert [(f, list(n)) for f, n in again["calls"]] == [(f, list(n)) for f, n in st["calls"]]   # the same tick, the same calls


# 2
def test_step_and_min_tasks(monkeypatch):
    t = cycle_tick()
    monkeypatch.setenv("SWP_STREAM_GROUP_TASKS", "128")
    st = run_streamed(t, 0)
    assert [f + len(n) for f, n in st["calls"]] == host_marks(t.sizes, 128)      # the calls are the host rule's marks
    check_all(t, st, plain_of(t))
    st = run_streamed(t, 300)
    assert len(st["calls"]) >= 2
    check_all(t, st, plain_of(t), 300)
    monkeypatch.delenv("SWP_STREAM_GROUP_TASKS")
    small = Tick("cycle, first 12 groups", t.nodes, t.services, t.groups[:12])    # 1 + 63 + 64 + 65 + 100, twice, + 1 + 63: below 1024
    assert small.total < 1024
    st = run_streamed(small, 0)
    assert [(f, len(n)) for f, n in st["calls"]] == [(0, small.total)]           # the default step with a total below it: one range
    check_all(small, st, plain_of(small))


# 3
def test_the_mirror_holds_a_range_when_the_sink_sees_it(monkeypatch):
    monkeypatch.setenv("SWP_STREAM_GROUP_TASKS", "128")
    t = cycle_tick()
    s0, _ = engine_of(t)
    N = len(t.nodes)
    start = s0.e.node_get_many(np.arange(N, dtype=np.uint32))
    cpu, mem, total = start["cpu"].astype(np.int64).copy(), start["mem"].astype(np.int64).copy(), start["total"].astype(np.int64).copy()
    svc_count = {}
    checked = [0]

    def inside(s, descs, calls):
        first, nodes = calls[-1]
        group_of = np.searchsorted(t.ends, np.arange(first, first + len(nodes)), side="right")
        for i, n in enumerate(nodes):   # the host replay of the ranges so far
            if n >= 0:
                d = descs[group_of[i]]
                cpu[n] -= int(d["cpu"])
                mem[n] -= int(d["mem"])
                total[n] += 1
                svc_count[(int(n), int(d["service"]))] = svc_count.get((int(n), int(d["service"])), 0) + 1
        for i, n in enumerate(nodes):
            if n < 0:
                continue
            row = s.e.node_get(int(n))
            assert (row.cpu, row.mem, row.total) == (cpu[n], mem[n], total[n]), (first, int(n))
            svc = int(descs[group_of[i]]["service"])
            assert s.e.node_get_svc_count(int(n), svc) == svc_count[(int(n), svc)]
            checked[0] += 1
        return False
    st = run_streamed(t, 0, inside)
    assert checked[0] > 0 and len(st["calls"]) >= 3
    check_all(t, st, plain_of(t))


# 4
def leftovers_tick():
    """tests/test_engine_groups.py test_spread_with_constraints_and_leftovers: two spread levels, a constraint, tight memory — some
    groups are only partly placed; the one-off tasks with preferences are groups of one"""
    nodes = [sc.node("n%02d" % i, Spec={"Annotations": {"Labels": {"az": "az%d" % (i % 3), "rack": "r%d" % (i % 5), "tier": "a" if i % 4 else "b"}}},
                     Description={"Resources": {"NanoCPUs": int(4e9), "MemoryBytes": int((1 + i % 3) * 1e9)}}) for i in range(40)]
    prefs = [{"Spread": {"SpreadDescriptor": "node.labels.az"}}, {"Spread": {"SpreadDescriptor": "node.labels.rack"}}]
    groups = [(group_doc("svcA", 1, Placement={"Preferences": prefs, "Constraints": ["node.labels.tier==a"]}, Resources={"Reservations": {"MemoryBytes": int(6e8)}}), 70),
              (group_doc("svcB", 1, Placement={"Preferences": prefs[:1], "MaxReplicas": 2}, Resources={"Reservations": {"MemoryBytes": int(3e8)}}), 50)]
    groups += [(group_doc("svcC", None, Placement={"Preferences": prefs[1:]}), 1) for _ in range(30)]
    groups += [(group_doc("svcD", 1, Placement={"Preferences": prefs}, Resources={"Reservations": {"MemoryBytes": int(6e8)}}), 40)]
    return Tick("spread, constraints, leftovers", nodes, ["svcA", "svcB", "svcC", "svcD"], groups)


def test_spread_preferences_with_resources_and_leftovers(monkeypatch):
    monkeypatch.setenv("SWP_STREAM_GROUP_TASKS", "1")
    t = leftovers_tick()
    st = run_streamed(t, 0)
    seen = np.concatenate([n for _, n in st["calls"]])
    assert (seen == -1).any() and (seen >= 0).any()                      # -1 arrives in the stream
    left = [g for g in range(len(t.groups)) if (st["out"][t.ends[g] - t.sizes[g]:t.ends[g]] < 0).any()]
    assert left and all(st["hist"][g].sum() > 0 for g in left)           # the histograms are complete at return
    assert len(st["calls"]) == len(t.groups)
    check_all(t, st, plain_of(t))


# 5
def non_bulk_tick():
    """groups with host ports and generic reservations among plain ones: what the bulk fold does not take (uncounted tasks: the test
    behind this one)"""
    nodes = [node_doc(i, {"az": "az%d" % (i % 2)}, generic=(sc.discrete("gpu", 1 + i % 4) + (sc.discrete("fpga", 2) if i % 2 else [])) if i % 3 != 2 else None) for i in range(90)]
    svcs = ["svc%d" % k for k in range(27)]   # (a service per group: tasks a group leaves over are tried again, and must not join a later group)
    groups = []
    for g in range(27):
        spec = {"Resources": {"Reservations": {"NanoCPUs": 10**8, "MemoryBytes": 64 << 20}}}
        if g % 3 == 1:
            spec["Resources"]["Reservations"]["Generic"] = sc.discrete("gpu", 1 + g % 2) + (sc.discrete("fpga", 1) if g % 2 else [])
        doc = group_doc(svcs[g], 1, **spec)
        if g % 5 == 0:
            doc["Endpoint"] = {"Ports": [{"PublishMode": 1, "Protocol": 0, "PublishedPort": 8000 + g, "TargetPort": 80}]}
        groups.append((doc, 5 + 7 * (g % 6)))
    return Tick("ports, generic, 27 groups x 90 nodes", nodes, svcs, groups)


def test_the_non_bulk_fold(monkeypatch):
    monkeypatch.setenv("SWP_STREAM_GROUP_TASKS", "16")
    t = non_bulk_tick()
    kinds = ("gpu", "fpga")
    st = run_streamed(t, 0, kinds=kinds)
    d = st["descs"]
    assert (d["port_set"] != 0).any() and (d["generic_set"] != 0).any()
    assert len(st["calls"]) >= 5
    check_all(t, st, plain_of(t, kinds=kinds))     # counts: the generic and per-service counts of every node against the twin's


def test_uncounted_tasks_fold_like_the_twin(monkeypatch):
    """SWP_TASK flag 0x2 (a task that does not count on its node) has no document form the oracle shares: against the twin only."""
    monkeypatch.setenv("SWP_STREAM_GROUP_TASKS", "1")
    t = Tick("uncounted groups", [node_doc(i) for i in range(70)], ["svc0", "svc1"],
             [(group_doc("svc%d" % (g % 2), 1, Resources={"Reservations": {"MemoryBytes": 32 << 20}}), 9 + g) for g in range(8)])

    def run(streamed):
        s, descs = engine_of(t)
        descs["flags"][::2] |= abi.TASK_UNCOUNTED
        calls = []
        out, hist = s.e.schedule_groups_streamed(descs, t.sizes, lambda f, n: calls.append((f, n.copy())) and False) if streamed else s.e.schedule_groups(descs, t.sizes)
        return out, hist, all_rows(s, 70), counts_of(s, t, descs), calls
    a, b = run(True), run(False)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2] == b[2] and a[3] == b[3]
    check_ranges(t, a[4], 0)
    assert len(a[4]) == 8


# 6
def mounts_tick():
    rng = random.Random(0x6057)
    zones = ["z1", "z2", "z3"]
    nodes, vols, groups = [], [], []
    for i in range(40):
        csi = []
        for plug in ("p1", "p2"):
            if rng.random() < 0.8:
                cd = {"PluginName": plug}
                if rng.random() < 0.8:
                    cd["AccessibleTopology"] = {"Segments": {"zone": rng.choice(zones)}}
                csi.append(cd)
        nodes.append({"ID": "n%04d" % i, "Status": {"State": orc.READY}, "Spec": {"Annotations": {"Labels": {"zone": rng.choice(zones)}}},
                      "Description": {"Resources": {"NanoCPUs": 8 * 10**9, "MemoryBytes": 16 << 30}, "CSIInfo": csi}})
    for v in range(12):
        acc = [{"Segments": {"zone": rng.choice(zones)}} for _ in range(rng.choice([0, 1, 1, 2]))]
        vols.append({"ID": "vol%02d" % v, "Spec": {"Annotations": {"Name": "name%02d" % v}, "Group": rng.choice(["", "g1", "g2"]), "Driver": {"Name": rng.choice(["p1", "p2"])},
                                                   "AccessMode": {"Scope": rng.choice([kv.SINGLE, kv.MULTI]), "Sharing": rng.choice([kv.NONE, kv.READ_ONLY, kv.ONE_WRITER, kv.ALL])},
                                                   "Availability": "ACTIVE"},
                     "VolumeInfo": {"VolumeID": "csi%02d" % v, "AccessibleTopology": acc}})
    for g in range(24):
        spec = {}
        if g % 2 == 0:
            spec["Container"] = {"Mounts": [kv.cluster_mount(rng.choice(["name%02d" % rng.randrange(13), "group:" + rng.choice(["g1", "g2", "g9"])]), rng.choice(["/a", "/b", "/c"]), rng.random() < 0.4)
                                            for _ in range(rng.choice([1, 1, 2, 3]))]}
        if g % 3 == 0:
            spec["Resources"] = {"Reservations": {"NanoCPUs": rng.choice([1, 2]) * 10**8, "MemoryBytes": 64 << 20}}
        groups.append((group_doc("svc%d" % g, 1, **spec), rng.choice([1, 3, 8, 20])))
    return Tick("mounts 24 groups x 40 nodes", nodes, ["svc%d" % k for k in range(24)], groups, vols)


def test_cluster_mounts(monkeypatch):
    monkeypatch.setenv("SWP_STREAM_GROUP_TASKS", "1")
    t = mounts_tick()
    st = run_streamed(t, 0, want_att=True)
    plain = plain_of(t, volumes=True)
    assert (st["att"] != abi.NO_VOLUME).any()            # some task got a volume: the attachments compared below are not all empty
    assert (st["att"] == plain["att"]).all()
    check_all(t, st, plain)
    for v in range(12):                                  # the volumes' usage as the tick left it
        assert st["s"].volume_info("vol%02d" % v)["Engine"] == plain["s"].volume_info("vol%02d" % v)["Engine"], v
    again = run_streamed(t, 0, want_att=False)           # out_att = NULL is accepted
    assert (again["out"] == plain["out"]).all() and again["rows"] == plain["rows"]


# 7
def test_the_global_memory_arena(monkeypatch):
    """One group, among LDS-sized ones, whose working set exceeds the LDS arena (G2_ARENA_LDS = 122 880 bytes): 3 200 tasks on 3 200 nodes
    without spread preferences — g2_arena_bytes(S = 3200 slots, 1 tree node, 0 generic kinds, depth 0, k = 3200)
    = 32 * 3200 + 64 * 2 + 8 * (2 + 51) + 4 * (2 * 3200 + 6) + 64 = 128 640 bytes."""
    monkeypatch.setenv("SWP_STREAM_GROUP_TASKS", "1")
    nodes = [node_doc(i, cpu=4, mem_gb=4 + i % 3) for i in range(3200)]
    res = {"Reservations": {"NanoCPUs": 10**8, "MemoryBytes": 256 << 20}}
    groups = [(group_doc("svc0", 1, Resources=res), 50), (group_doc("svc1", 1, Resources=res), 3200), (group_doc("svc2", 1, Resources=res), 70), (group_doc("svc1", 1, Resources=res), 33)]
    t = Tick("3200 nodes, a group of 3200", nodes, ["svc0", "svc1", "svc2"], groups)
    st = run_streamed(t, 0)
    assert [len(n) for _, n in st["calls"]] == [50, 3200, 70, 33]
    check_all(t, st, plain_of(t))


# 8
def test_edges(monkeypatch):
    monkeypatch.setenv("SWP_STREAM_GROUP_TASKS", "1")
    t = cycle_tick()
    s, descs = engine_of(t)
    calls = []
    out, hist = s.e.schedule_groups_streamed(descs[:0], t.sizes[:0], lambda f, n: calls.append(f))
    assert len(out) == 0 and calls == []                                 # n_groups 0: no call
    one = Tick("one group of 1", t.nodes, t.services, [(t.groups[0][0], 1)])
    st = run_streamed(one, 0)
    assert [(f, len(n)) for f, n in st["calls"]] == [(0, 1)]
    check_all(one, st, plain_of(one))
    empty = Tick("no nodes", [], t.services, t.groups[:3])
    st = run_streamed(empty, 0)
    assert [(f, list(n)) for f, n in st["calls"]] == [(0, [-1] * empty.total)]   # the empty nodeSet's answer, as one range
    assert (st["out"] == -1).all() and (st["hist"] == 0).all()
    p = plain_of(empty)
    assert (p["out"] == st["out"]).all() and (p["hist"] == st["hist"]).all()
    with pytest.raises(abi.SwpError) as ei:                              # an argument check of the plain call: an empty group
        s.e.schedule_groups_streamed(descs[:2], np.array([3, 0], dtype=np.uint32), lambda f, n: calls.append(f))
    assert ei.value.code == abi.SWP_EINVAL and calls == []


# 9
def cancel_tick():
    """4 000 groups of 4 on 256 nodes; every other group reserves a generic resource"""
    nodes = [node_doc(i, generic=sc.discrete("gpu", 24 + 8 * (i % 3)), cpu=64, mem_gb=256) for i in range(256)]
    svcs = ["svc%d" % k for k in range(8)]
    plain = {"Resources": {"Reservations": {"NanoCPUs": 10**7, "MemoryBytes": 8 << 20}}}
    gen = {"Resources": {"Reservations": {"NanoCPUs": 10**7, "MemoryBytes": 8 << 20, "Generic": sc.discrete("gpu", 1)}}}
    groups = [(group_doc(svcs[g % 8], 1, **(gen if g % 2 else plain)), 4) for g in range(4000)]
    return Tick("cancel 4000 groups of 4 x 256 nodes", nodes, svcs, groups)


def test_cancel_takes_everything_back(monkeypatch):
    monkeypatch.setenv("SWP_STREAM_GROUP_TASKS", "1")
    t = cancel_tick()
    s, descs = engine_of(t)
    N = len(t.nodes)
    before, counts_before = all_rows(s, N), counts_of(s, t, descs, ("gpu",))
    calls = []

    def sink(first, nodes):
        calls.append((first, len(nodes)))
        return len(calls) == 2
    with pytest.raises(abi.SwpError) as ei:
        s.e.schedule_groups_streamed(descs, t.sizes, sink, 0)
    assert ei.value.code == abi.SWP_ECANCELLED and len(calls) == 2
    m = re.search(r"the kernel stopped after group (\d+) of 4000", ei.value.msg)
    print(ei.value.msg)
    assert m and int(m.group(1)) < 4000, ei.value.msg
    assert all_rows(s, N) == before                                      # every node row ...
    assert counts_of(s, t, descs, ("gpu",)) == counts_before             # ... per-service count and generic count as snapshotted
    out, hist = s.e.schedule_groups(descs, t.sizes)                      # the same tick, plainly, from the state as it was
    plain = plain_of(t, kinds=("gpu",))
    assert (out == plain["out"]).all() and (hist == plain["hist"]).all() and all_rows(s, N) == plain["rows"]
    assert counts_of(s, t, descs, ("gpu",)) == plain["counts"]
    check_oracle(t, s, out, hist)


# 10
def test_a_shard_set_refuses():
    wl = synth.Workload("cfg3", T=100, N=40, services=5)
    s = swhost.HostScheduler(shards=2, nodes_per_shard=20)
    descs = swhost.load_workload(s, wl)
    sizes = np.array([20, 30, 50], dtype=np.uint32)
    out = np.full(100, 12345, dtype=np.int32)
    hist = np.full((3, abi.NFILTERS), 777, dtype=np.uint32)
    called = []
    cb = abi.PREFIX_SINK(lambda ctx, first, count, nodes: called.append(first) or 0)
    rc = s.e.L.swp_schedule_groups_streamed(s.e.h, descs[:3].ctypes.data, sizes.ctypes.data, 3, out.ctypes.data, hist.ctypes.data, None, cb, None, 0)
    assert rc == abi.SWP_EUNSUPPORTED and not called and (out == 12345).all() and (hist == 777).all()


# 11
def test_the_streamed_instance_ships_and_passes_the_kernel_checks():
    abi.build_library()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_kernels.py"), "--verbose"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    lines = {name: [l for l in r.stdout.splitlines() if " %s " % name in l] for name in ("k_groups2", "k_groups2s")}
    assert len(lines["k_groups2"]) == 1 and len(lines["k_groups2s"]) == 1, r.stdout
    assert " wg  1024 " in lines["k_groups2s"][0]
