"""GPU: one-off tasks with spread preferences INSIDE a batch (csrc/swp_scan_spread.hpp, k_scan_spread: a batch's spread segments) against
the oracle (tests/orc.py), decision for decision, "no suitable node (...)" strings included.

The engine side is driven through the struct ABI with NO host split in between: a tick's one-off tasks go down as ONE batch, in the
oracle's task order, the tasks with preferences in their places (WholeRun below: the Python twin of the host layer, tests/pyhost.py, with
the splitting loop taken out — everything else of it, the node mirror, the bookings, the Explain strings, as it is). Afterwards the node
rows and the per-service counts are read back (swp_node_get, swp_node_get_svc_count) and compared, and a second tick runs on that state.
On the parent commit every such batch is refused with SWP_EUNSUPPORTED.

The host layer's opt-in (SWP_SCHED_ONEOFF_SPREAD=1, csrc/swp_sched.cpp) is tested at the end, through the product's own scheduler.
The CPU side of the kernel — its source on fibers against a model of the reference's text — is tests/test_emu_scan_spread.py."""
import os
import random

import numpy as np
import pytest

import orc
import pyhost
import scenarios as sc
from swarmkit_amd import abi
from swarmkit_amd import host as swhost

pytestmark = pytest.mark.gpu
GIB = 1 << 30
MIB = 1 << 20


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    for k in ("SWP_R6_BLOCK", "SWP_STREAM_EVERY", "SWP_SCAN", "SWP_WATERFILL", "SWP_SCHED_ONEOFF_SPREAD", "SWP_HOST"):
        monkeypatch.delenv(k, raising=False)


class WholeRun(pyhost.PyHostScheduler):
    """The host layer without the split: a tick's one-off tasks are ONE device call. mode: which entry takes it."""

    def __init__(self, mode="batch", **kw):
        super().__init__(**kw)
        self.mode, self.calls, self.ranges = mode, 0, []

    def _schedule_queue(self, queue, decisions):
        grouped, run = {}, []
        for tid, t in queue:
            if t.get("SpecVersion") is not None:
                grouped.setdefault((t.get("ServiceID", ""), pyhost._get(t, "SpecVersion", "Index", default=0)), []).append((tid, t))
            else:
                run.append((tid, t, self.task_desc(t)))
        self._run_groups(list(grouped.values()), decisions)
        self._run_one_offs(run, decisions)

    def _run_one_offs(self, run, decisions):   # (no handler: a refusal is the test's failure, not a deferred task)
        if not run:
            return
        descs = np.concatenate([d for _, _, d in run])
        self.calls += 1
        if self.mode == "batch":
            out, hist = self.e.schedule_batch(descs)
        elif self.mode == "prepared":
            b = self.e.batch_prepare(descs)
            b.run()
            out, hist = b.fetch()
            b.free()
        elif self.mode == "templates":
            uniq, inverse = np.unique(descs, return_inverse=True)
            b = self.e.batch_prepare_templates(uniq, inverse.astype(np.uint32))
            b.run()
            out, hist = b.fetch()
            b.free()
        else:
            seen = []
            out, hist = self.e.schedule_batch_streamed(descs, lambda first, nodes: seen.append((first, nodes.copy())) and False, 0)
            at = 0
            for first, nodes in seen:
                assert first == at and len(nodes) > 0
                assert (nodes == out[first:first + len(nodes)]).all()
                at += len(nodes)
            assert at == len(descs)
            self.ranges.append(len(seen))
        for (tid, t, _), n, h in zip(run, out, hist):
            if n >= 0:
                self._place(tid, t, n, decisions)
            else:
                self._no_suitable_node(tid, t, h, decisions)
        self._push_touched()


def key(d):
    return (d["ID"], d["NodeID"], d["Err"], d["State"], str(d.get("AssignedGenericResources") or ""))


_oracle_cache = {}


def oracle_of(name, events):
    """([sorted decisions of every tick], {node id: node info at the end}) — computed once per script and left unchanged."""
    if name not in _oracle_cache:
        o, ticks, ids = orc.Oracle(), [], []
        for ev in events:
            if ev[0] == "tick":
                ticks.append(sorted(key(d) for d in o.tick()))
            else:
                getattr(o, ev[0])(*ev[1:])
                if ev[0] == "create_node":
                    ids.append(ev[1]["ID"])
        _oracle_cache[name] = (ticks, {i: o.node_info(i) for i in ids})
    return _oracle_cache[name]


def rows_equal(want, e):
    for nid, a in want.items():
        b = e.node_info(nid)
        assert a["ActiveTasksCount"] == b["ActiveTasksCount"], nid
        assert a["AvailableResources"]["NanoCPUs"] == b["AvailableResources"]["NanoCPUs"], nid
        assert a["AvailableResources"]["MemoryBytes"] == b["AvailableResources"]["MemoryBytes"], nid
        assert {k: v for k, v in a["ActiveTasksCountByService"].items() if v} == b["ActiveTasksCountByService"], nid


def run_script(name, events, mode="batch"):
    want_ticks, want_rows = oracle_of(name, events)
    e, k = WholeRun(mode), 0
    for ev in events:
        if ev[0] == "tick":
            got = sorted(key(d) for d in e.tick())
            assert got == want_ticks[k], (name, k, [(a, b) for a, b in zip(want_ticks[k], got) if a != b][:5])
            k += 1
        else:
            getattr(e, ev[0])(*ev[1:])
    rows_equal(want_rows, e)
    return e


def spread(*keys):
    return [{"Spread": {"SpreadDescriptor": k}} for k in keys]


def node(i, labels, cpu=4, mem_gib=4, ready=True, **kw):
    return sc.node("n%05d" % i, Spec={"Annotations": {"Labels": labels}}, Status={"State": orc.READY if ready else orc.DOWN},
                   Description={"Resources": dict({"NanoCPUs": cpu * 10**9, "MemoryBytes": int(mem_gib * GIB)}, **kw)})


def running(tid, service, node_id, **kw):
    return dict({"ID": tid, "ServiceID": service, "NodeID": node_id, "DesiredState": orc.RUNNING, "Status": {"State": orc.RUNNING}}, **kw)


# ------------------------------------------------------------------------------------------------------------------ the shapes
def shape_one_leaf():
    """Preferences that create no level (nodeset.go:79-80: only label descriptors do) next to tasks without any: trees of one leaf."""
    ev = [("create_node", node(i, {"zone": "z%d" % (i % 3)}, mem_gib=1 + i % 2)) for i in range(40)]
    ev += [("set_service", "a"), ("set_service", "b")]
    for j in range(90):
        ev.append(("create_task", sc.pending("a%03d" % j, "a", Spec={"Placement": {"Preferences": spread("node.hostname")}, "Resources": {"Reservations": {"MemoryBytes": 700 * MIB}}})))
        ev.append(("create_task", sc.pending("b%03d" % j, "b", Spec={"Placement": {"Preferences": spread("node.labels.zone")}})))
    return ev + [("tick",), ("tick",)]


def shape_no_room():
    """One level; zone c holds no feasible node (a constraint): its tasks leave tasksInUsableBranches, the others share what is left."""
    ev = [("create_node", node(i, {"zone": "abc"[i % 3], "disk": "hdd" if i % 3 == 2 else "ssd"})) for i in range(60)]
    ev += [("set_service", "a")]
    for j in range(5):   # the branch without room carries tasks of the service
        ev.append(("create_task", running("r%d" % j, "a", "n%05d" % (2 + 3 * j))))
    for j in range(100):
        ev.append(("create_task", sc.pending("a%03d" % j, "a", Spec={"Placement": {"Preferences": spread("node.labels.zone"), "Constraints": ["node.labels.disk==ssd"]}})))
    return ev + [("tick",), ("create_task", sc.pending("z", "a", Spec={"Placement": {"Preferences": spread("node.labels.zone")}})), ("tick",)]


def shape_not_ready_branch():
    """A branch whose nodes are all down but carry tasks of the service: they count in tree.tasks (nodeset.go:88-90) and never take one."""
    ev = [("create_node", node(i, {"zone": "abc"[i % 3]}, ready=i % 3 != 1)) for i in range(45)]
    ev += [("set_service", "a"), ("set_service", "b")]
    for j in range(12):
        ev.append(("create_task", running("r%02d" % j, "a", "n%05d" % (1 + 3 * (j % 7)))))
    for j in range(40):
        ev.append(("create_task", sc.pending("a%03d" % j, "a", Spec={"Placement": {"Preferences": spread("node.labels.zone")}})))
        ev.append(("create_task", sc.pending("b%03d" % j, "b")))
    return ev + [("tick",), ("tick",)]


def shape_missing_label():
    ev = [("create_node", node(i, {"zone": "ab"[i % 2]} if i % 5 else ({} if i % 2 else {"rack": "r1"}))) for i in range(70)]
    ev += [("set_service", "a")]
    for j in range(150):
        ev.append(("create_task", sc.pending("a%03d" % j, "a", Spec={"Placement": {"Preferences": spread("node.labels.zone", "node.labels.rack")},
                                                                    "Resources": {"Reservations": {"NanoCPUs": 2 * 10**9}}})))
    return ev + [("tick",), ("tick",)]


def shape_xy():
    """The two-level shape: dc X = racks A (2 tasks of the service) and B (none), dc Y = 10 tasks; ONE new task. The root hands X
    desired - tasks + 1 = 5 tasks, and inside X rack A (2 < 3) is visited first and takes the one there is."""
    ev = []
    for i in range(45):
        dc, rack = ("X", "A") if i < 15 else ("X", "B") if i < 30 else ("Y", "C")
        ev.append(("create_node", node(i, {"dc": dc, "rack": rack})))
    ev += [("set_service", "a")]
    for j in range(2):
        ev.append(("create_task", running("xa%d" % j, "a", "n%05d" % j)))
    for j in range(10):
        ev.append(("create_task", running("y%02d" % j, "a", "n%05d" % (30 + j))))
    ev.append(("create_task", sc.pending("new", "a", Spec={"Placement": {"Preferences": spread("node.labels.dc", "node.labels.rack")}})))
    return ev + [("tick",), ("tick",)]


def shape_three_levels():
    ev = [("create_node", node(i, {"az": "az%d" % (i % 3), "rack": "r%d" % (i % 5), "tier": "ab"[i % 4 == 0]}, mem_gib=1 + i % 3)) for i in range(120)]
    ev += [("set_service", "a"), ("set_service", "b"), ("set_service", "c")]
    for j in range(140):
        ev.append(("create_task", sc.pending("a%03d" % j, "a", Spec={"Placement": {"Preferences": spread("node.labels.az", "node.labels.rack", "node.labels.tier")},
                                                                    "Resources": {"Reservations": {"MemoryBytes": 1500 * MIB}}})))
        if j % 2:
            ev.append(("create_task", sc.pending("b%03d" % j, "b", Spec={"Placement": {"Preferences": spread("node.labels.tier", "node.labels.az"), "MaxReplicas": 1}})))
        if j % 3 == 0:
            ev.append(("create_task", sc.pending("c%03d" % j, "c", Spec={"Resources": {"Reservations": {"MemoryBytes": 900 * MIB}}})))
    return ev + [("tick",), ("tick",)]


def shape_history():
    """Services that already run on nodes, five recent failures on some (scheduler.go:711-721), MaxReplicas, a task that is not counted
    (DesiredState beyond COMPLETE), host ports, generic reservations, and reservations tight enough that tasks find no node."""
    ev = []
    for i in range(80):
        gen = sc.discrete("gpu", i % 3) if i % 4 else []
        ev.append(("create_node", node(i, {"zone": "abcd"[i % 4], "rack": "r%d" % (i % 3)}, mem_gib=1 + i % 2, Generic=gen)))
    for s in "abcde":
        ev.append(("set_service", s))
    for j in range(30):
        ev.append(("create_task", running("ra%02d" % j, "a", "n%05d" % (j * 2 % 80))))
    fail = []
    for j in range(12):   # six failures of service b on each of two nodes
        t = running("fb%02d" % j, "b", "n%05d" % (4 if j < 6 else 9))
        ev.append(("create_task", t))
        fail.append(("update_task", dict(t, Status={"State": orc.FAILED})))
    ev += fail
    port = {"Ports": [{"Protocol": 0, "PublishedPort": 8080, "PublishMode": 1}]}
    for j in range(60):
        ev.append(("create_task", sc.pending("a%03d" % j, "a", Spec={"Placement": {"Preferences": spread("node.labels.zone"), "MaxReplicas": 1}})))
        ev.append(("create_task", sc.pending("b%03d" % j, "b", Spec={"Placement": {"Preferences": spread("node.labels.zone", "node.labels.rack")},
                                                                    "Resources": {"Reservations": {"MemoryBytes": 1500 * MIB}}})))
        ev.append(("create_task", sc.pending("c%03d" % j, "c", Spec={"Placement": {"Preferences": spread("node.labels.rack")}}, Endpoint=port)))
        ev.append(("create_task", sc.pending("d%03d" % j, "d", Spec={"Placement": {"Preferences": spread("node.labels.zone")},
                                                                    "Resources": {"Reservations": {"Generic": sc.discrete("gpu", 2)}}})))
        if j % 6 == 0:
            ev.append(("create_task", dict(sc.pending("e%03d" % j, "e", Spec={"Placement": {"Preferences": spread("node.labels.zone")}}), DesiredState=orc.SHUTDOWN)))
    return ev + [("tick",), ("tick",)]


def shape_large(n_nodes, n_tasks):
    rng = random.Random(n_nodes)
    ev = [("create_node", node(i, {"zone": "z%d" % rng.randrange(6), "rack": "r%d" % rng.randrange(5)}, mem_gib=rng.choice([1, 2, 4]), ready=rng.random() < 0.97)) for i in range(n_nodes)]
    ev += [("set_service", "a"), ("set_service", "b")]
    for j in range(n_tasks):
        if j % 3:
            ev.append(("create_task", sc.pending("a%04d" % j, "a", Spec={"Placement": {"Preferences": spread("node.labels.zone", "node.labels.rack")},
                                                                       "Resources": {"Reservations": {"MemoryBytes": 900 * MIB}}})))
        else:
            ev.append(("create_task", sc.pending("b%04d" % j, "b", Spec={"Placement": {"Preferences": spread("node.labels.rack")}})))
    return ev + [("tick",), ("create_task", sc.pending("last", "b", Spec={"Placement": {"Preferences": spread("node.labels.rack")}})), ("tick",)]


def shape_mixed():
    """Plain tasks, then spread, then plain, then spread — stretches long enough for the block resolver to stand in front of, between and
    behind the segments (swp_rounds.hpp SPREAD_GAP) —, one service with and without preferences, a spread task first and last."""
    ev = [("create_node", node(i, {"zone": "abc"[i % 3]}, mem_gib=2 + i % 2)) for i in range(150)]
    ev += [("set_service", "a"), ("set_service", "b")]
    pref = {"Placement": {"Preferences": spread("node.labels.zone")}}
    res = {"Resources": {"Reservations": {"MemoryBytes": 500 * MIB}}}
    ev.append(("create_task", sc.pending("first", "a", Spec=pref)))
    for j in range(130):
        ev.append(("create_task", sc.pending("p1%03d" % j, "ab"[j % 2], Spec=res)))
    for j in range(40):
        ev.append(("create_task", sc.pending("s1%03d" % j, "a", Spec=dict(pref, **res) if j % 2 else pref)))
        if j % 10 == 0:
            ev.append(("create_task", sc.pending("q1%03d" % j, "a", Spec=res)))   # (rides along in the segment)
    for j in range(200):
        ev.append(("create_task", sc.pending("p2%03d" % j, "ab"[j % 2], Spec=res)))
    for j in range(30):
        ev.append(("create_task", sc.pending("s2%03d" % j, "b", Spec=pref)))
    ev.append(("create_task", sc.pending("zlast", "a", Spec=pref)))
    return ev + [("tick",), ("tick",)]


SHAPES = {
    "one_leaf": shape_one_leaf, "no_room": shape_no_room, "not_ready_branch": shape_not_ready_branch, "missing_label": shape_missing_label, "xy": shape_xy,
    "three_levels": shape_three_levels, "history": shape_history, "mixed": shape_mixed, "n1025": lambda: shape_large(1025, 300), "n4096": lambda: shape_large(4096, 400),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_one_batch_against_the_oracle(name):
    e = run_script(name, SHAPES[name]())
    assert e.calls >= 1


def test_the_branch_that_is_handed_five_picks_rack_a():
    """The oracle's own answer for the two-level shape: the node of rack A with the fewest tasks — not rack B, which a walk that hands
    down one task would choose."""
    ticks, _ = oracle_of("xy", shape_xy())
    (tid, nid, err, state, _), = ticks[0]
    assert tid == "new" and not err and int(nid[1:]) < 15, ticks[0]


def test_mixed_batch_has_segments_and_rounds():
    e2 = WholeRun()   # (the first tick alone: the counters are the last batch's)
    for ev in shape_mixed():
        if ev[0] == "tick":
            e2.tick()
            break
        getattr(e2, ev[0])(*ev[1:])
    st = e2.e.stats()
    assert st["scan_launches"] >= 3 and st["scan_tasks"] >= 76, st   # the spread segments (counted with the scan stretches): 1 + 44 + 31 tasks ...
    assert st["resolve_launches"] > 0, st                            # ... and rounds of the block resolver for the plain stretches


@pytest.mark.parametrize("mode", ["prepared", "templates", "streamed"])
@pytest.mark.parametrize("name", ["history", "mixed"])
def test_prepared_and_streamed_entries(name, mode):
    e = run_script(name, SHAPES[name](), mode)
    if mode == "streamed":
        assert e.ranges and e.ranges[0] >= (3 if name == "mixed" else 1), e.ranges


def test_streamed_ranges_are_in_the_mirror_when_the_sink_sees_them():
    ev = [x for x in shape_mixed() if x[0] != "tick"]
    e = WholeRun()
    for x in ev:
        getattr(e, x[0])(*x[1:])
    queue = [(tid, t) for tid, t in e.unassigned.items()]
    descs = np.concatenate([e.task_desc(t) for _, t in queue])
    n = 150
    before = np.array([e.e.node_get(i).total for i in range(n)])
    counts, seen = np.zeros(n, dtype=np.int64), []

    def sink(first, nodes):
        seen.append((first, len(nodes)))
        for x in nodes:
            if x >= 0:
                counts[x] += 1
        for i in set(int(x) for x in nodes if x >= 0):
            assert e.e.node_get(i).total == before[i] + counts[i], (first, i)
        return False
    out, _ = e.e.schedule_batch_streamed(descs, sink, 0)
    at = 0
    for first, cnt in seen:
        assert first == at
        at += cnt
    assert at == len(descs) and len(seen) >= 3
    twin = WholeRun()
    for x in ev:
        getattr(twin, x[0])(*x[1:])
    plain, _ = twin.e.schedule_batch(np.concatenate([twin.task_desc(t) for _, t in queue]))   # (its own descriptors: the ids are the engine's)
    assert (plain == out).all()


# ------------------------------------------------------------------------------------------------------------------ fuzz
KEYS = ["zone", "rack", "tier"]


def fuzz_script(seed):
    """(events, facts): N <= 300 nodes, T <= 600 one-off tasks over two ticks, 0 - 3 spread levels over 2 - 3 label keys of 1 - 6 values,
    constraints, reservations tight enough that tasks stay unplaced, generic reservations, host ports, MaxReplicas, services that already
    run. A node's description never changes. facts: the ids of the tasks with preferences, and whether some service spreads over a key
    one of whose values its constraint rules out while nodes carry it (a branch without room whenever the walk visits it)."""
    rng = random.Random(0x5EED + seed)
    n_nodes = rng.choice([40, 64, 65, 120, 200, 300])
    n_keys = rng.choice([2, 3])
    vals = [rng.randrange(1, 7) for _ in range(n_keys)]
    ev, have = [], [set() for _ in range(n_keys)]
    for i in range(n_nodes):
        labels = {}
        for k in range(n_keys):
            if rng.random() < 0.9:
                labels[KEYS[k]] = "v%d" % rng.randrange(vals[k])
                have[k].add(labels[KEYS[k]])
        gen = sc.discrete("gpu", rng.randrange(1, 4)) if rng.random() < 0.5 else []
        ev.append(("create_node", node(i, labels, cpu=rng.choice([2, 4, 8]), mem_gib=rng.choice([1, 2, 4]), ready=rng.random() < 0.93, Generic=gen)))
    n_svc = rng.randrange(1, 8)
    specs, spreads, no_room = [], [], False
    for s in range(n_svc):
        ev.append(("set_service", "svc%d" % s))
        levels = rng.sample(range(n_keys), rng.randrange(0, n_keys + 1))
        pl, spec, doc = {}, {}, {}
        if levels:
            pl["Preferences"] = spread(*["node.labels." + KEYS[k] for k in levels])
        r = rng.random()
        if r < 0.3:
            k = levels[0] if levels and rng.random() < 0.7 else rng.randrange(n_keys)
            v = "v%d" % rng.randrange(vals[k])
            pl["Constraints"] = ["node.labels.%s!=%s" % (KEYS[k], v)]
            no_room = no_room or (bool(levels) and k == levels[0] and v in have[k] and len(have[k]) > 1)
        elif r < 0.4:
            pl["Constraints"] = ["node.labels.%s==v0" % KEYS[rng.randrange(n_keys)]]
        if rng.random() < 0.2:
            pl["MaxReplicas"] = rng.choice([1, 2, 3])
        res = {}
        if rng.random() < 0.7:
            res = {"NanoCPUs": rng.choice([0, 500, 1000, 2000]) * 10**6, "MemoryBytes": rng.choice([0, 256, 700, 1500]) * MIB}
        if rng.random() < 0.2:
            res["Generic"] = sc.discrete("gpu", rng.choice([1, 2]))
        if res:
            spec["Resources"] = {"Reservations": res}
        if pl:
            spec["Placement"] = pl
        if spec:
            doc["Spec"] = spec
        if rng.random() < 0.15:
            doc["Endpoint"] = {"Ports": [{"Protocol": 0, "PublishedPort": 9000 + rng.randrange(3), "PublishMode": 1}]}
        specs.append(doc)
        spreads.append(bool(levels))
        for j in range(rng.choice([0, 0, 3, 20])):   # the service runs already
            ev.append(("create_task", running("run%d_%d" % (s, j), "svc%d" % s, "n%05d" % rng.randrange(n_nodes))))
    with_prefs, tid = set(), 0
    for tick in range(2):
        for _ in range(rng.randrange(1, 6)):
            s = rng.randrange(n_svc)
            for _ in range(rng.choice([1, 3, 10, 30, 60])):
                t = dict(sc.pending("t%05d" % tid, "svc%d" % s), **specs[s])
                if spreads[s] and rng.random() < 0.1:   # one service with and without preferences
                    t = dict(t, Spec=dict(t["Spec"], Placement={k: v for k, v in t["Spec"]["Placement"].items() if k != "Preferences"}))
                elif spreads[s]:
                    with_prefs.add(t["ID"])
                ev.append(("create_task", t))
                tid += 1
        ev.append(("tick",))
    return ev, dict(with_prefs=with_prefs, no_room=no_room and bool(with_prefs))


FIRST, SEEDS = int(os.environ.get("SWP_FUZZ_FIRST", "0")), int(os.environ.get("SWP_FUZZ_SEEDS", "64"))


@pytest.mark.parametrize("seed", range(FIRST, FIRST + SEEDS))
def test_fuzz(seed):
    ev, _ = fuzz_script(seed)
    run_script("fuzz%d" % seed, ev)


def test_fuzz_seeds_cover_the_ground():
    """Over the seeds: some task with preferences is placed, some is left without a node, some seed has a branch without room — from the
    oracle's answers and the scripts alone."""
    placed = unplaced = no_room = 0
    for seed in range(FIRST, FIRST + SEEDS):
        ev, facts = fuzz_script(seed)
        ticks, _ = oracle_of("fuzz%d" % seed, ev)
        for tid, nid, err, state, _ in (d for t in ticks for d in t):
            if tid in facts["with_prefs"]:
                if nid and state >= orc.ASSIGNED:
                    placed += 1
                elif err.startswith("no suitable node"):
                    unplaced += 1
        no_room += facts["no_room"]
    if SEEDS >= 64:
        assert placed and unplaced and no_room, (placed, unplaced, no_room)


# ------------------------------------------------------------------------------------------------------------------ limits
def test_beyond_4096_node_slots_the_refusal_stays():
    e = WholeRun()
    for i in range(4097):
        e.create_node(node(i, {"zone": "ab"[i % 2]}))
    e.set_service("a")
    d_spread = e.task_desc(sc.pending("t1", "a", Spec={"Placement": {"Preferences": spread("node.labels.zone")}}))
    d_plain = e.task_desc(sc.pending("t2", "a"))
    rows = e.e.node_get_many(np.arange(4097, dtype=np.uint32)).tobytes()
    for call in (e.e.schedule_batch, e.e.batch_prepare, lambda d: e.e.schedule_batch_streamed(d, lambda *a: False)):
        with pytest.raises(abi.SwpError) as err:
            call(np.concatenate([d_plain, d_spread]))
        assert err.value.code == abi.SWP_EUNSUPPORTED and "4096" in str(err.value) and "swp_schedule_groups" in str(err.value)
    assert e.e.node_get_many(np.arange(4097, dtype=np.uint32)).tobytes() == rows
    out, _ = e.e.schedule_batch(d_plain)   # (and the engine goes on)
    assert out[0] == 0


def test_a_spread_task_with_cluster_mounts_is_refused(monkeypatch):
    monkeypatch.setenv("SWP_HOST", "cxx")   # (the product's host layer: the twin takes no cluster mounts)
    s = swhost.HostScheduler()
    for i in range(8):
        s.create_node(node(i, {"zone": "ab"[i % 2]}))
    s.set_service("a")
    t = sc.pending("t1", "a", Spec={"Placement": {"Preferences": spread("node.labels.zone")}, "Container": {"Mounts": [{"Type": 4, "Source": "vol0", "Target": "/m"}]}})
    d = s.task_desc(t)
    assert int(d["spread_set"][0]) and int(d["flags"][0]) >> 8
    rows = s.e.node_get_many(np.arange(8, dtype=np.uint32)).tobytes()
    with pytest.raises(abi.SwpError) as err:
        s.e.schedule_batch(d)
    assert err.value.code == abi.SWP_EUNSUPPORTED and "cluster mounts" in str(err.value)
    assert s.e.node_get_many(np.arange(8, dtype=np.uint32)).tobytes() == rows


def test_a_shard_set_refuses_as_before(monkeypatch):
    monkeypatch.setenv("SWP_HOST", "cxx")
    s = swhost.HostScheduler(shards=3, nodes_per_shard=10)
    for i in range(24):
        s.create_node(node(i, {"zone": "ab"[i % 2]}))
    s.set_service("a")
    d = s.task_desc(sc.pending("t1", "a", Spec={"Placement": {"Preferences": spread("node.labels.zone")}}))
    with pytest.raises(abi.SwpError) as err:
        s.e.schedule_batch(d)
    assert err.value.code == abi.SWP_EUNSUPPORTED and "swp_schedule_groups" in str(err.value)


# ------------------------------------------------------------------------------------------------------------------ the host layer
def groups_script():
    """The event script of tests/test_engine_groups.py::test_spread_with_constraints_and_leftovers (30 one-off tasks with preferences)."""
    ev = []
    for i in range(40):
        ev.append(("create_node", sc.node(f"n{i:02d}", Spec={"Annotations": {"Labels": {"az": f"az{i % 3}", "rack": f"r{i % 5}", "tier": "a" if i % 4 else "b"}}},
                                          Description={"Resources": {"NanoCPUs": int(4e9), "MemoryBytes": int((1 + i % 3) * 1e9)}})))
    for sname in ("svcA", "svcB", "svcC"):
        ev.append(("set_service", sname))
    prefs = spread("node.labels.az", "node.labels.rack")
    for i in range(70):
        ev.append(("create_task", sc.pending(f"a{i:03d}", "svcA", 1, Spec={"Placement": {"Preferences": prefs, "Constraints": ["node.labels.tier==a"]},
                                                                         "Resources": {"Reservations": {"MemoryBytes": int(6e8)}}})))
    for i in range(50):
        ev.append(("create_task", sc.pending(f"b{i:03d}", "svcB", 2, Spec={"Placement": {"Preferences": prefs[:1], "MaxReplicas": 2},
                                                                         "Resources": {"Reservations": {"MemoryBytes": int(3e8)}}})))
    for i in range(30):
        ev.append(("create_task", sc.pending(f"c{i:03d}", "svcC", Spec={"Placement": {"Preferences": prefs[1:]}})))
    return ev + [("tick",), ("tick",)]


@pytest.mark.parametrize("name", ["groups_script", "fuzz3", "history"])
def test_host_layer_keeps_spread_one_offs_in_the_run(monkeypatch, name):
    monkeypatch.setenv("SWP_HOST", "cxx")
    monkeypatch.setenv("SWP_SCHED_ONEOFF_SPREAD", "1")
    ev = groups_script() if name == "groups_script" else fuzz_script(3)[0] if name == "fuzz3" else shape_history()
    want_ticks, want_rows = oracle_of(name if name != "groups_script" else "groups_script", ev)
    s, k = swhost.HostScheduler(), 0
    for x in ev:
        if x[0] == "tick":
            b0 = s.e.stats()["batches"]
            got = sorted(key(d) for d in s.tick())
            assert got == want_ticks[k], (name, k, [(a, b) for a, b in zip(want_ticks[k], got) if a != b][:5])
            if name == "groups_script" and k == 0:
                st = s.e.stats()   # the call for the two task groups, then ONE batch with a spread segment over the 30 tasks — not 30 calls for groups of one
                assert st["batches"] == b0 + 2 and st["scan_tasks"] == 30 and st["scan_launches"] == 1, st
            k += 1
        else:
            getattr(s, x[0])(*x[1:])
    for nid, a in want_rows.items():
        b = s.node_info(nid)
        assert a["ActiveTasksCount"] == b["ActiveTasksCount"] and a["AvailableResources"]["MemoryBytes"] == b["AvailableResources"]["MemoryBytes"], nid


def test_without_the_knob_the_host_layer_splits_as_before(monkeypatch):
    monkeypatch.setenv("SWP_HOST", "cxx")
    ev = groups_script()
    want_ticks, _ = oracle_of("groups_script", ev)
    s = swhost.HostScheduler()
    for x in ev[:-1]:
        if x[0] == "tick":
            assert sorted(key(d) for d in s.tick()) == want_ticks[0]
            assert s.e.stats()["batches"] == 31   # (the two task groups in one call; every one-off task of the script has preferences: 30 calls for groups of one)
        else:
            getattr(s, x[0])(*x[1:])
