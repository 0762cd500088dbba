"""GPU: one-off tasks with spread preferences and NO constraint inside a batch on a nodeSet of more than 4 096 node slots — a task whose
own class row holds every ready node (csrc/swp_scan_spread.hpp k_scan_spread_wide: all node slots, the node rows in global memory;
csrc/swp_engine.hip spread_cut: with SWP_SPREAD_WIDE=1 a segment that cannot be cut runs whole through it) — against the oracle
(tests/orc.py), decision for decision, "no suitable node (...)" strings included.

The driver, the comparison and the helpers are those of tests/test_engine_oneoff_spread.py and its two successors (WholeRun: a tick's
one-off tasks go down as ONE batch, no host split; afterwards every node's row and per-service counts are compared, and a second tick
runs on that state). 4 200 node slots, at most 400 tasks. On the parent commit every oracle comparison here is refused with
SWP_EUNSUPPORTED; test_without_the_switch_the_refusal_stays passes there too.

The CPU side of the kernel — its source on fibers against a model over all nodes — is tests/test_emu_scan_spread_wide.py."""
import os
import random

import numpy as np
import pytest

import orc
import scenarios as sc
from swarmkit_amd import abi
from swarmkit_amd import host as swhost
from test_engine_oneoff_spread import MIB, WholeRun, key, node, oracle_of, run_script, running, spread
from test_engine_oneoff_spread_compact import first_tick, loaded, placements, pool_nodes, pooled
from test_engine_oneoff_spread_cut import shape_riders

pytestmark = pytest.mark.gpu
N = 4200
ZONES = 5
WIDE_MAXN = 65536   # csrc/swp_scan_spread.hpp SPREAD_WIDE_MAXN


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    for k in ("SWP_R6_BLOCK", "SWP_STREAM_EVERY", "SWP_SCAN", "SWP_WATERFILL", "SWP_SCHED_ONEOFF_SPREAD", "SWP_HOST", "SWP_SCANB_COMPACT", "SWP_SCAN_UNBATCHED", "SWP_DBG"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SWP_SPREAD_WIDE", "1")   # (read once, when the engine is created)


def free(tid, service, prefs=("node.labels.zone",), mem=0, **placement):
    """A pending task with preferences and no constraint: its class row holds every ready node."""
    pl = dict(placement)
    if prefs:
        pl["Preferences"] = spread(*prefs)
    spec = {"Placement": pl}
    if mem:
        spec["Resources"] = {"Reservations": {"MemoryBytes": mem * MIB}}
    return sc.pending(tid, service, Spec=spec)


# ------------------------------------------------------------------------------------------------------------------ the shapes
UNCONSTRAINED_TASKS = 360


def shape_unconstrained():
    """Two services spreading over the zone on all 4 200 nodes. Service a reserves 1 500 MiB and every 21st node only has 2 GiB (the
    others 1 GiB): 200 such nodes, 240 tasks — 40 find no node. Service b runs with and without preferences."""
    ev = [("create_node", node(i, {"zone": "z%d" % (i * 7 % ZONES)}, mem_gib=2 if i % 21 == 0 else 1)) for i in range(N)]
    ev += [("set_service", "a"), ("set_service", "b")]
    for j in range(12):   # service b runs already, all in one zone
        ev.append(("create_task", running("r%02d" % j, "b", "n%05d" % (5 * j))))
    for j in range(UNCONSTRAINED_TASKS // 3):
        ev.append(("create_task", free("a%03d" % (2 * j), "a", mem=1500)))
        ev.append(("create_task", free("b%03d" % j, "b", prefs=("node.labels.zone",) if j % 9 else ())))
        ev.append(("create_task", free("a%03d" % (2 * j + 1), "a", mem=1500)))
    return ev + [("tick",), ("create_task", free("last", "b")), ("create_task", free("lasta", "a", mem=1500)), ("tick",)]


MIXED_TASKS = 300


def shape_mixed():
    """Pooled spread tasks (a pool of 300) and unconstrained spread tasks alternate in ONE segment: the whole segment runs wide."""
    ev = pool_nodes() + [("set_service", "a"), ("set_service", "b"), ("set_service", "c")]
    for j in range(MIXED_TASKS // 3):
        ev.append(("create_task", pooled("a%03d" % j, "a", mem=300 if j % 2 else 0)))
        ev.append(("create_task", free("b%03d" % j, "b", mem=700)))
        ev.append(("create_task", free("c%03d" % j, "c") if j % 4 else sc.pending("c%03d" % j, "c")))   # (a plain task rides along)
    return ev + [("tick",), ("create_task", pooled("u0", "a")), ("create_task", free("u1", "b", mem=700)), ("tick",)]


def shape_wide_and_compact():
    """A pooled segment (compact), 70 plain tasks constrained to the pool (more than the 64 that end a segment), an unconstrained one (wide)."""
    ev = pool_nodes() + [("set_service", "a"), ("set_service", "b"), ("set_service", "c")]
    for j in range(40):
        ev.append(("create_task", pooled("s1%03d" % j, "a", mem=300 if j % 2 else 0)))
    for j in range(70):
        ev.append(("create_task", pooled("p%03d" % j, "c", prefs=(), mem=200)))
    for j in range(40):
        ev.append(("create_task", free("s2%03d" % j, "b", mem=600)))
    return ev + [("tick",), ("tick",)]


SHAPES = {"unconstrained": shape_unconstrained, "mixed": shape_mixed, "wide_and_compact": shape_wide_and_compact}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_one_batch_against_the_oracle(name):
    e = run_script("wide_" + name, SHAPES[name]())
    assert e.calls == (1 if name == "wide_and_compact" else 2)


def test_unconstrained_leaves_tasks_without_a_node():
    """(CPU: the oracle alone.) The script is as tight as it says: tasks of service a find no node, with the reason."""
    ticks, _ = oracle_of("wide_unconstrained", shape_unconstrained())
    errs = [err for tid, nid, err, state, _ in ticks[0] if not nid]
    assert len(errs) == 40 and all(e.startswith("no suitable node (") for e in errs), errs[:3]


def test_unconstrained_is_one_launch():
    st = first_tick(shape_unconstrained()).e.stats()
    assert st["scan_tasks"] == UNCONSTRAINED_TASKS and st["scan_launches"] == 1, st
    assert st["resolve_launches"] == 0, st


def test_mixed_is_one_launch():
    st = first_tick(shape_mixed()).e.stats()
    assert st["scan_tasks"] == MIXED_TASKS and st["scan_launches"] == 1, st


def test_riders_stay_cut():
    """No own row is too wide: the segment is cut exactly as without the switch, the riders go to the block resolver."""
    e = run_script("cut_riders", shape_riders())
    assert e.calls == 2
    st = first_tick(shape_riders()).e.stats()
    assert st["resolve_launches"] > 0 and st["scan_launches"] >= 44, st


def test_wide_and_compact_name_their_instances(monkeypatch, capfd):
    monkeypatch.setenv("SWP_DBG", "16")
    st = first_tick(shape_wide_and_compact()).e.stats()
    err = capfd.readouterr().err
    assert "k_scan_spread decided tasks [0, 40) over a union of 300 of 4200 nodes" in err, err[-2000:]
    assert "k_scan_spread_wide decided tasks [110, 150) over all 4200 node slots" in err, err[-2000:]
    assert st["scan_launches"] >= 2, st


@pytest.mark.parametrize("mode", ["prepared", "templates", "streamed"])
@pytest.mark.parametrize("name", ["unconstrained", "mixed"])
def test_prepared_and_streamed_entries(name, mode):
    e = run_script("wide_" + name, SHAPES[name](), mode)
    if mode == "streamed":   # (WholeRun asserts that the ranges tile [0, T))
        assert e.ranges and e.ranges[0] >= 1, e.ranges


# ------------------------------------------------------------------------------------------------------------------ limits
def test_a_label_that_moves_between_prepare_and_run():
    """Prepared on `unconstrained`; a fifth of the nodes move to a zone that did not exist (a sixth branch). The run is never refused for
    its width: it succeeds, on trees built from the labels as they are now."""
    ev = shape_unconstrained()
    ev = ev[:ev.index(("tick",))]
    moved = [("create_node", node(i, {"zone": "znew"}, mem_gib=2 if i % 21 == 0 else 1)) for i in range(0, N, 5)]
    e, descs = loaded(ev)
    b = e.e.batch_prepare(descs)
    for x in moved:
        e.create_node(x[1])
    b.run()
    out, _ = b.fetch()
    b.free()
    nodes_ev = [x for x in ev if x[0] == "create_node"]
    rest = [x for x in ev if x[0] != "create_node"]
    want, _ = oracle_of("wide_unconstrained_moved", nodes_ev + moved + rest + [("tick",)])
    ids = [tid for tid, _ in e.unassigned.items()]
    got = {tid: ("n%05d" % n if n >= 0 else "") for tid, n in zip(ids, out)}
    assert got == placements(want)
    assert any(int(nid[1:]) % 5 == 0 for nid in got.values() if nid)   # (the new zone takes tasks)


def bulk_engine(n):
    """An engine with n ready nodes of five zones, created through the node call alone (no host mirror: no oracle is asked)."""
    e = WholeRun()
    e.create_node(node(0, {"zone": "z0"}, mem_gib=1))
    doc = node(0, {"zone": "z0"}, mem_gib=1)
    zones = []
    for z in range(ZONES):
        _, lab, _, _ = e._node_row(node(0, {"zone": "z%d" % z}, mem_gib=1), 0, 4 * 10**9, 1 << 30, 0)
        zones.append(lab)
    row, _, elab, plugins = e._node_row(doc, 0, 4 * 10**9, 1 << 30, 0)
    for i in range(1, n):
        nid = "n%05d" % i
        row.node = e.e.intern(abi.SPACE_NODE_ID, nid)
        row.id_fold = e._folded(nid)
        e.e.node_upsert(row, zones[i % ZONES], elab, plugins)
    return e


def test_beyond_65536_node_slots_is_refused():
    e = bulk_engine(WIDE_MAXN + 1)
    e.set_service("a")
    descs = np.concatenate([e.task_desc(free("t%02d" % j, "a")) for j in range(10)])
    every = np.arange(WIDE_MAXN + 1, dtype=np.uint32)
    rows = e.e.node_get_many(every).tobytes()
    for call in (e.e.schedule_batch, e.e.batch_prepare, lambda d: e.e.schedule_batch_streamed(d, lambda *a: False)):
        with pytest.raises(abi.SwpError) as err:
            call(descs)
        assert err.value.code == abi.SWP_EUNSUPPORTED and "65536" in str(err.value) and "swp_schedule_groups" in str(err.value), str(err.value)
    assert e.e.node_get_many(every).tobytes() == rows
    out, _ = e.e.schedule_batch(e.task_desc(sc.pending("plain", "a")))   # (and the engine goes on)
    assert out[0] >= 0


def test_without_the_switch_the_refusal_stays(monkeypatch):
    """(Passes on the parent commit too: the message is the parent's, word for word.)"""
    monkeypatch.delenv("SWP_SPREAD_WIDE")
    ev = shape_unconstrained()
    e, descs = loaded(ev[:ev.index(("tick",))])
    every = np.arange(N, dtype=np.uint32)
    rows = e.e.node_get_many(every).tobytes()
    for call in (e.e.schedule_batch, e.e.batch_prepare, lambda d: e.e.schedule_batch_streamed(d, lambda *a: False)):
        with pytest.raises(abi.SwpError) as err:
            call(descs)
        assert err.value.code == abi.SWP_EUNSUPPORTED
        assert ("a task has spread preferences: schedule it through swp_schedule_groups (a batch takes them where the nodes its segment's tasks can use number at most 4096: "
                "the union of the class rows of segment 0, tasks [0, %d), has 4200 of this nodeSet's 4200)" % UNCONSTRAINED_TASKS) in str(err.value), str(err.value)
    assert e.e.node_get_many(every).tobytes() == rows


# ------------------------------------------------------------------------------------------------------------------ fuzz
KEYS = ["zone", "rack", "tier"]


def fuzz_script(seed):
    """(events, facts): 4 097 - 4 400 nodes (even seeds: at least 4 160, of which at most 40 are not ready, and a service with levels
    and no constraint), a pool of 50 - 2 500 nodes; services pooled and unconstrained with 0 - 3 spread levels over 2 - 3 label keys of
    1 - 5 values, each label missing on a tenth of the nodes; services that run already; reservations tight enough that tasks stay
    unplaced, MaxReplicas, host ports, generic reservations; at most 400 tasks over two ticks.
    facts: `own_row` — a task with preferences whose own class row has more than 4 096 ready nodes, from the script alone."""
    rng = random.Random(0x71DE + seed)
    even = seed % 2 == 0
    n_nodes = rng.randrange(4160, 4401) if even else rng.randrange(4097, 4401)
    n_keys = rng.choice([2, 3])
    vals = [rng.randrange(1, 6) for _ in range(n_keys)]
    down = set(rng.sample(range(n_nodes), rng.randrange(0, 41) if even else rng.randrange(0, 200)))
    pool = set(rng.sample(range(n_nodes), rng.choice([50, 300, 1000, 2500])))
    ev = []
    for i in range(n_nodes):
        labels = {}
        for k in range(n_keys):
            if rng.random() < 0.9:
                labels[KEYS[k]] = "v%d" % rng.randrange(vals[k])
        if i in pool:
            labels["pool"] = "1"
        gen = sc.discrete("gpu", rng.randrange(1, 4)) if rng.random() < 0.5 else []
        mem_gib = 8 if rng.random() < 0.01 else rng.choice([1, 2, 4])   # (some forty nodes that take a reservation of 5 000 MiB: one each)
        ev.append(("create_node", node(i, labels, cpu=rng.choice([2, 4, 8]), mem_gib=mem_gib, ready=i not in down, Generic=gen)))
    ready = n_nodes - len(down)
    n_svc = rng.randrange(2, 7)
    specs, wide = [], []   # wide[s]: the service's tasks have preferences and an own row of more than 4 096 ready nodes
    for s in range(n_svc):
        ev.append(("set_service", "svc%d" % s))
        pooled_svc = rng.random() < 0.4 and not (even and s == 0)
        levels = rng.sample(range(n_keys), rng.randrange(0, n_keys + 1))
        if even and s == 0 and not levels:
            levels = [rng.randrange(n_keys)]
        pl, spec, doc = {}, {}, {}
        if pooled_svc:
            pl["Constraints"] = ["node.labels.pool==1"]
        if levels:
            pl["Preferences"] = spread(*["node.labels." + KEYS[k] for k in levels])
        if rng.random() < 0.2:
            pl["MaxReplicas"] = rng.choice([1, 2, 3])
        res = {}
        if rng.random() < 0.7:
            res = {"NanoCPUs": rng.choice([0, 500, 1000, 2000]) * 10**6, "MemoryBytes": rng.choice([0, 256, 700, 3000, 5000, 5000]) * MIB}
        if rng.random() < 0.2:
            res["Generic"] = sc.discrete("gpu", rng.choice([1, 2, 3]))
        if res:
            spec["Resources"] = {"Reservations": res}
        spec["Placement"] = pl
        doc["Spec"] = spec
        if rng.random() < 0.15:
            doc["Endpoint"] = {"Ports": [{"Protocol": 0, "PublishedPort": 9000 + rng.randrange(3), "PublishMode": 1}]}
        specs.append(doc)
        wide.append(bool(levels) and not pooled_svc and ready > 4096)
        for j in range(rng.choice([0, 3, 20, 40])):   # the service runs already
            ev.append(("create_task", running("run%d_%d" % (s, j), "svc%d" % s, "n%05d" % rng.randrange(n_nodes))))
    own_row, tid, left = False, 0, 400
    for tick in range(2):
        for r in range(rng.randrange(1, 6)):
            s = 0 if even and tick == 0 and r == 0 else rng.randrange(n_svc)
            for _ in range(min(left, rng.choice([1, 3, 10, 30, 60, 100]))):
                t = dict(sc.pending("t%05d" % tid, "svc%d" % s), **specs[s])
                if wide[s] and rng.random() < 0.1 and tid:   # one service with and without preferences
                    t = dict(t, Spec=dict(t["Spec"], Placement={k: v for k, v in t["Spec"]["Placement"].items() if k != "Preferences"}))
                elif wide[s]:
                    own_row = True
                ev.append(("create_task", t))
                tid += 1
                left -= 1
        ev.append(("tick",))
    return ev, dict(own_row=own_row)


FIRST, SEEDS = int(os.environ.get("SWP_FUZZ_FIRST", "0")), int(os.environ.get("SWP_FUZZ_SEEDS", "32"))


@pytest.mark.parametrize("seed", range(FIRST, FIRST + SEEDS))
def test_fuzz(seed):
    ev, _ = fuzz_script(seed)
    run_script("wide_fuzz%d" % seed, ev)


def test_fuzz_seeds_cover_the_ground():
    """(CPU: the scripts alone.) At least half of the seeds hold a task with preferences whose own row has more than 4 096 ready nodes."""
    own = sum(fuzz_script(seed)[1]["own_row"] for seed in range(FIRST, FIRST + SEEDS))
    assert own >= (SEEDS + 1) // 2, own
    if SEEDS >= 32:
        assert own >= 16, own


# ------------------------------------------------------------------------------------------------------------------ the host layer
HOST_ONE_OFFS = 60


def host_script():
    """A task group (a SpecVersion) and 60 unconstrained one-off tasks with preferences, on 4 200 nodes."""
    ev = [("create_node", node(i, {"zone": "z%d" % (i * 7 % ZONES)}, mem_gib=1 + i % 3)) for i in range(N)]
    ev += [("set_service", s) for s in ("a", "b", "g")]
    for i in range(40):
        ev.append(("create_task", sc.pending("g%03d" % i, "g", 1, Spec={"Resources": {"Reservations": {"MemoryBytes": 600 * MIB}}})))
    for j in range(8):   # service b runs already, in one zone
        ev.append(("create_task", running("rb%d" % j, "b", "n%05d" % (5 + 70 * j))))
    for j in range(HOST_ONE_OFFS):
        ev.append(("create_task", free("t%03d" % j, "ab"[j % 2], mem=2500 if j % 2 == 0 else 0)))
    return ev + [("tick",), ("create_task", free("u0", "b")), ("tick",)]


def host_run(ev, name, on_first_tick):
    want_ticks, want_rows = oracle_of(name, ev)
    s, k = swhost.HostScheduler(), 0
    for x in ev:
        if x[0] == "tick":
            b0 = s.e.stats()["batches"]
            got = sorted(key(d) for d in s.tick())
            assert got == want_ticks[k], (k, [(a, b) for a, b in zip(want_ticks[k], got) if a != b][:5])
            if k == 0:
                on_first_tick(s.e.stats(), b0)
            k += 1
        else:
            getattr(s, x[0])(*x[1:])
    for nid, a in want_rows.items():
        b = s.node_info(nid)
        assert a["ActiveTasksCount"] == b["ActiveTasksCount"] and a["AvailableResources"]["MemoryBytes"] == b["AvailableResources"]["MemoryBytes"], nid


def test_host_layer_keeps_the_tick_one_batch(monkeypatch):
    monkeypatch.setenv("SWP_HOST", "cxx")
    monkeypatch.setenv("SWP_SCHED_ONEOFF_SPREAD", "1")

    def check(st, b0):   # the call for the task group, then ONE batch: one wide segment
        assert st["batches"] == b0 + 2, st
        assert st["scan_launches"] == 1 and st["scan_tasks"] == HOST_ONE_OFFS, st

    host_run(host_script(), "wide_host", check)


def test_without_the_switch_the_host_layer_splits_as_the_parent_does(monkeypatch):
    monkeypatch.setenv("SWP_HOST", "cxx")
    monkeypatch.setenv("SWP_SCHED_ONEOFF_SPREAD", "1")
    monkeypatch.delenv("SWP_SPREAD_WIDE")

    def check(st, b0):   # the call for the task group; the batch is refused at its preparation; a call for a group of one per task
        assert st["batches"] == b0 + 1 + HOST_ONE_OFFS, st
        assert st["scan_launches"] == 0, st

    host_run(host_script(), "wide_host", check)
