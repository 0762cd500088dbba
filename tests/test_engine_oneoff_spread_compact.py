"""GPU: one-off tasks with spread preferences inside a batch on a nodeSet of MORE than 4 096 node slots (csrc/swp_scan_spread.hpp,
k_scan_spread<.., true>: a spread segment over the union of its tasks' class rows, with the base sums of the nodes outside that union
from k_spread_base) against the oracle (tests/orc.py), decision for decision, "no suitable node (...)" strings included.

The driver, the comparison and the helpers are those of tests/test_engine_oneoff_spread.py (WholeRun: a tick's one-off tasks go down as
ONE batch, no host split; afterwards every node's row and per-service counts are compared, and a second tick runs on that state). The
shapes are the smallest that can go wrong: 4 200 node slots, pools of a few hundred nodes, at most 400 tasks. On the parent commit every
such batch is refused with SWP_EUNSUPPORTED ("... at most 4096 node slots ...").

The CPU side of the kernels — their source on fibers against a model over all nodes — is tests/test_emu_scan_spread_compact.py."""
import os
import random

import numpy as np
import pytest

import orc
import scenarios as sc
from swarmkit_amd import abi
from swarmkit_amd import host as swhost
from test_engine_oneoff_spread import MIB, WholeRun, key, node, oracle_of, run_script, running, spread

pytestmark = pytest.mark.gpu
N = 4200
ZONES = 5


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    for k in ("SWP_R6_BLOCK", "SWP_STREAM_EVERY", "SWP_SCAN", "SWP_WATERFILL", "SWP_SCHED_ONEOFF_SPREAD", "SWP_HOST", "SWP_SCANB_COMPACT", "SWP_SCAN_UNBATCHED"):
        monkeypatch.delenv(k, raising=False)


def in_pool(i, every=14, phase=0):
    return i % every == phase


def pool_nodes(zone_of=lambda i: "z%d" % (i * 7 % ZONES), pools=(("a", 14, 0),), mem_gib=lambda i: 1 + (i // 14 + i) % 2):
    """N nodes; node i carries pool=<name> when i % every == phase for one of `pools` (the first that matches), and a zone."""
    ev = []
    for i in range(N):
        labels = {"zone": zone_of(i)}
        for name, every, phase in pools:
            if in_pool(i, every, phase):
                labels["pool"] = name
                break
        ev.append(("create_node", node(i, labels, mem_gib=mem_gib(i))))
    return ev


def pooled(tid, service, pool="a", prefs=("node.labels.zone",), mem=0, **placement):
    pl = dict({"Constraints": ["node.labels.pool==%s" % pool]}, **placement)
    if prefs:
        pl["Preferences"] = spread(*prefs)
    spec = {"Placement": pl}
    if mem:
        spec["Resources"] = {"Reservations": {"MemoryBytes": mem * MIB}}
    return sc.pending(tid, service, Spec=spec)


# ------------------------------------------------------------------------------------------------------------------ the shapes
def shape_pool():
    """Services constrained to a pool every 14th node carries (300 of 4 200), spreading over the zone; reservations tight enough that
    tasks of one service are left without a node; one service with and without preferences."""
    ev = pool_nodes() + [("set_service", "a"), ("set_service", "b")]
    for j in range(180):
        ev.append(("create_task", pooled("a%03d" % j, "a", mem=1500)))   # (the pool's 150 nodes of 2 GiB take one each)
        ev.append(("create_task", pooled("b%03d" % j, "b", prefs=("node.labels.zone",) if j % 9 else ())))
    return ev + [("tick",), ("create_task", pooled("last", "b")), ("tick",)]


def shape_outside_counts(with_running=True):
    """Running tasks of the service on nodes OUTSIDE the pool, all in zone z0 — a zone the pool has nodes in too: the branch starts heavy."""
    ev = pool_nodes() + [("set_service", "a")]
    if with_running:
        at = 0
        for i in range(N):
            if at < 40 and not in_pool(i) and i * 7 % ZONES == 0:
                ev.append(("create_task", running("r%02d" % at, "a", "n%05d" % i)))
                at += 1
        assert at == 40
    for j in range(120):
        ev.append(("create_task", pooled("a%03d" % j, "a")))
    return ev + [("tick",), ("create_task", pooled("last", "a")), ("tick",)]


def shape_outside_branch():
    """A zone that exists only outside the pool and carries tasks of the service: a branch the walk finds without room."""
    ev = pool_nodes(zone_of=lambda i: "zx" if i % 14 == 3 else "z%d" % (i * 7 % ZONES)) + [("set_service", "a"), ("set_service", "b")]
    for j in range(6):
        ev.append(("create_task", running("r%d" % j, "a", "n%05d" % (3 + 14 * j))))
    for j in range(100):
        ev.append(("create_task", pooled("a%03d" % j, "a")))
        ev.append(("create_task", pooled("b%03d" % j, "b", mem=600)))
    return ev + [("tick",), ("create_task", pooled("last", "a")), ("tick",)]


def shape_two_pools():
    """Plain (unconstrained: the whole cluster), spread in pool a, plain, spread in pool b: another union per segment, the block resolver
    in between — it places tasks of the segments' services on nodes outside the next segment's union."""
    ev = pool_nodes(pools=(("a", 14, 0), ("b", 21, 5))) + [("set_service", "a"), ("set_service", "b")]
    res = {"Resources": {"Reservations": {"MemoryBytes": 300 * MIB}}}
    for j in range(130):
        ev.append(("create_task", sc.pending("p1%03d" % j, "ab"[j % 2], Spec=res)))
    for j in range(40):
        ev.append(("create_task", pooled("s1%03d" % j, "a", "a", mem=300 if j % 2 else 0)))
    for j in range(200):
        ev.append(("create_task", sc.pending("p2%03d" % j, "ab"[j % 2], Spec=res)))
    for j in range(30):
        ev.append(("create_task", pooled("s2%03d" % j, "b", "b")))
    return ev + [("tick",), ("tick",)]


def shape_union(n_pool, tasks=200):
    """A pool of exactly n_pool of the 4 200 nodes (the nodes outside it are every 50th and then the last ones)."""
    out = set(range(0, N, 50))
    i = N - 1
    while N - len(out) > n_pool:
        out.add(i)
        i -= 1
    assert N - len(out) == n_pool
    ev = [("create_node", node(i, dict({"zone": "z%d" % (i * 7 % ZONES)}, **({} if i in out else {"pool": "a"})), mem_gib=1)) for i in range(N)]
    ev += [("set_service", "a"), ("set_service", "b")]
    for j in range(tasks // 2):
        ev.append(("create_task", pooled("a%03d" % j, "a")))
        ev.append(("create_task", pooled("b%03d" % j, "b", prefs=("node.labels.zone", "node.labels.pool"))))
    return ev + [("tick",), ("tick",)]


SHAPES = {"pool": shape_pool, "outside_counts": shape_outside_counts, "outside_branch": shape_outside_branch, "two_pools": shape_two_pools,
          "union_4096": lambda: shape_union(4096)}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_one_batch_against_the_oracle(name):
    e = run_script("compact_" + name, SHAPES[name]())
    assert e.calls >= 1


def placements(ticks, k=0):
    return {tid: nid for tid, nid, err, state, _ in ticks[k]}


def test_the_counts_outside_the_pool_change_the_answer():
    """The ORACLE's answer for `outside_counts` is not its answer without the running tasks outside the pool: a compaction that drops the
    nodes outside the union from the tree's sums computes the latter. (CPU: the oracle alone.)"""
    a, _ = oracle_of("compact_outside_counts", shape_outside_counts())
    b, _ = oracle_of("compact_outside_counts_without", shape_outside_counts(False))
    pa, pb = placements(a), placements(b)
    assert set(pa) == set(pb) and sum(pa[t] != pb[t] for t in pa) > 0
    z0 = lambda p: sum(1 for nid in p.values() if nid and int(nid[1:]) * 7 % ZONES == 0)
    assert z0(pa) < z0(pb), (z0(pa), z0(pb))   # (zone z0 carries 40 tasks of the service outside the pool: it is handed fewer)


def test_the_zone_outside_the_pool_takes_no_task():
    a, _ = oracle_of("compact_outside_branch", shape_outside_branch())
    assert all(nid and in_pool(int(nid[1:])) for tid, nid in placements(a).items() if tid.startswith("a"))


def first_tick(events, mode="batch"):
    e = WholeRun(mode)
    for ev in events:
        if ev[0] == "tick":
            e.tick()
            break
        getattr(e, ev[0])(*ev[1:])
    return e


def test_two_pools_has_segments_and_rounds():
    st = first_tick(shape_two_pools()).e.stats()
    assert st["scan_launches"] >= 2 and st["scan_tasks"] >= 70, st   # the two spread segments (counted with the scan stretches): 40 + 30 tasks ...
    assert st["resolve_launches"] > 0, st                            # ... and rounds of the block resolver for the plain stretches


@pytest.mark.parametrize("mode", ["prepared", "templates", "streamed"])
@pytest.mark.parametrize("name", ["pool", "two_pools"])
def test_prepared_and_streamed_entries(name, mode):
    e = run_script("compact_" + name, SHAPES[name](), mode)
    if mode == "streamed":   # (WholeRun asserts that the ranges tile [0, T))
        assert e.ranges and e.ranges[0] >= (3 if name == "two_pools" else 1), e.ranges


# ------------------------------------------------------------------------------------------------------------------ limits
def loaded(events):
    e = WholeRun()
    for ev in events:
        if ev[0] != "tick":
            getattr(e, ev[0])(*ev[1:])
    return e, np.concatenate([e.task_desc(t) for _, t in e.unassigned.items()])


def all_rows(e):
    return e.e.node_get_many(np.arange(N, dtype=np.uint32)).tobytes()


def test_a_pool_of_4097_is_refused():
    e, descs = loaded(shape_union(4097, tasks=20))
    rows = all_rows(e)
    for call in (e.e.schedule_batch, e.e.batch_prepare, lambda d: e.e.schedule_batch_streamed(d, lambda *a: False)):
        with pytest.raises(abi.SwpError) as err:
            call(descs)
        assert err.value.code == abi.SWP_EUNSUPPORTED and "4096" in str(err.value) and "swp_schedule_groups" in str(err.value) and "4097" in str(err.value)
    assert all_rows(e) == rows
    plain_task = e.task_desc(sc.pending("plain", "a"))   # (and the engine goes on)
    out, _ = e.e.schedule_batch(plain_task)
    assert out[0] >= 0


def test_a_label_that_moves_between_prepare_and_run():
    """Prepared on a pool of 4 096; one more node is labelled into the pool; the run is refused, rows unchanged. The label taken back, a
    fresh preparation runs."""
    ev = shape_union(4096, tasks=20)
    e, descs = loaded(ev)
    b = e.e.batch_prepare(descs)
    e.create_node(node(0, {"zone": "z0", "pool": "a"}, mem_gib=1))   # (node 0 is outside the pool)
    rows = all_rows(e)
    with pytest.raises(abi.SwpError) as err:
        b.run()
    assert err.value.code == abi.SWP_EUNSUPPORTED and "4096" in str(err.value) and "4097" in str(err.value)
    assert all_rows(e) == rows
    b.free()
    e.create_node(node(0, {"zone": "z0"}, mem_gib=1))
    b = e.e.batch_prepare(descs)
    b.run()
    out, _ = b.fetch()
    b.free()
    want, _ = oracle_of("compact_union_4096_20", ev)
    ids = [tid for tid, _ in e.unassigned.items()]
    assert {tid: ("n%05d" % n if n >= 0 else "") for tid, n in zip(ids, out)} == placements(want)


# ------------------------------------------------------------------------------------------------------------------ fuzz
KEYS = ["zone", "rack", "tier"]


def fuzz_script(seed):
    """(events, facts): 4 097 - 4 400 nodes, two pools of at most 400 nodes scattered over them, T <= 400 one-off tasks over two ticks,
    every service constrained to one pool (so that a segment's union stays small) with 0 - 3 spread levels over 2 - 3 label keys of 1 - 5
    values; some values exist only outside the pools; services run already, inside and outside their pool; reservations tight enough
    that tasks stay unplaced, MaxReplicas, host ports, generic reservations. A node's description never changes.
    facts: the ids of the tasks with preferences; whether a spreading service runs on a node outside its pool (non-zero outside counts);
    whether such a node sits in a first-level branch no node of the pool is in (a branch outside the union that carries tasks)."""
    rng = random.Random(0xC0AC7 + seed)
    n_nodes = rng.randrange(4097, 4401)
    n_keys = rng.choice([2, 3])
    vals = [rng.randrange(1, 6) for _ in range(n_keys)]
    sizes = [rng.choice([1, 40, 64, 65, 200, 400]), rng.choice([30, 150, 300])]
    order = list(range(n_nodes))
    rng.shuffle(order)
    pool_of = {}
    for n in order[:sizes[0]]:
        pool_of[n] = 0
    for n in order[sizes[0]:sizes[0] + sizes[1]]:
        pool_of[n] = 1
    ev, labels_of = [], []
    for i in range(n_nodes):
        labels = {}
        for k in range(n_keys):
            if rng.random() < 0.9:
                v = rng.randrange(vals[k] + (0 if i in pool_of else 1))   # (the value v<vals[k]> exists only outside the pools)
                labels[KEYS[k]] = "v%d" % v
        if i in pool_of:
            labels["pool"] = "p%d" % pool_of[i]
        labels_of.append(labels)
        gen = sc.discrete("gpu", rng.randrange(1, 4)) if rng.random() < 0.5 else []
        ev.append(("create_node", node(i, labels, cpu=rng.choice([2, 4, 8]), mem_gib=rng.choice([1, 2, 4]), ready=rng.random() < 0.95, Generic=gen)))
    outside = [i for i in range(n_nodes) if i not in pool_of]
    n_svc = rng.randrange(1, 7)
    specs, spreads, outside_counts, outside_branch = [], [], False, False
    for s in range(n_svc):
        ev.append(("set_service", "svc%d" % s))
        pool = rng.randrange(2)
        levels = rng.sample(range(n_keys), rng.randrange(0, n_keys + 1))
        pl, spec, doc = {"Constraints": ["node.labels.pool==p%d" % pool]}, {}, {}
        if levels:
            pl["Preferences"] = spread(*["node.labels." + KEYS[k] for k in levels])
        if rng.random() < 0.25:
            pl["Constraints"].append("node.labels.%s!=v%d" % (KEYS[rng.randrange(n_keys)], rng.randrange(3)))
        if rng.random() < 0.2:
            pl["MaxReplicas"] = rng.choice([1, 2, 3])
        res = {}
        if rng.random() < 0.7:
            res = {"NanoCPUs": rng.choice([0, 500, 1000, 2000]) * 10**6, "MemoryBytes": rng.choice([0, 256, 700, 1500]) * MIB}
        if rng.random() < 0.2:
            res["Generic"] = sc.discrete("gpu", rng.choice([1, 2]))
        if res:
            spec["Resources"] = {"Reservations": res}
        spec["Placement"] = pl
        doc["Spec"] = spec
        if rng.random() < 0.15:
            doc["Endpoint"] = {"Ports": [{"Protocol": 0, "PublishedPort": 9000 + rng.randrange(3), "PublishMode": 1}]}
        specs.append(doc)
        spreads.append(bool(levels))
        mine = [i for i, p in pool_of.items() if p == pool]
        for j in range(rng.choice([0, 3, 20, 40])):   # the service runs already: half of it outside its pool
            i = rng.choice(outside) if j % 2 else rng.choice(mine)
            ev.append(("create_task", running("run%d_%d" % (s, j), "svc%d" % s, "n%05d" % i)))
            if levels and j % 2:
                outside_counts = True
                k = KEYS[levels[0]]
                if labels_of[i].get(k, "") not in {labels_of[m].get(k, "") for m in mine}:
                    outside_branch = True
    with_prefs, tid, left = set(), 0, 400
    for tick in range(2):
        for _ in range(rng.randrange(1, 6)):
            s = rng.randrange(n_svc)
            for _ in range(min(left, rng.choice([1, 3, 10, 30, 60, 100]))):
                t = dict(sc.pending("t%05d" % tid, "svc%d" % s), **specs[s])
                if spreads[s] and rng.random() < 0.1:   # one service with and without preferences
                    t = dict(t, Spec=dict(t["Spec"], Placement={k: v for k, v in t["Spec"]["Placement"].items() if k != "Preferences"}))
                elif spreads[s]:
                    with_prefs.add(t["ID"])
                ev.append(("create_task", t))
                tid += 1
                left -= 1
        ev.append(("tick",))
    return ev, dict(with_prefs=with_prefs, outside_counts=outside_counts and bool(with_prefs), outside_branch=outside_branch and bool(with_prefs))


FIRST, SEEDS = int(os.environ.get("SWP_FUZZ_FIRST", "0")), int(os.environ.get("SWP_FUZZ_SEEDS", "32"))


@pytest.mark.parametrize("seed", range(FIRST, FIRST + SEEDS))
def test_fuzz(seed):
    ev, _ = fuzz_script(seed)
    run_script("compact_fuzz%d" % seed, ev)


def test_fuzz_seeds_cover_the_ground():
    """Over the seeds: some task with preferences is placed, some is left without a node, some seed has non-zero counts outside the union,
    some a branch outside the union that carries tasks — from the oracle's answers and the scripts alone."""
    placed = unplaced = counts = branch = 0
    for seed in range(FIRST, FIRST + SEEDS):
        ev, facts = fuzz_script(seed)
        ticks, _ = oracle_of("compact_fuzz%d" % seed, ev)
        for tid, nid, err, state, _ in (d for t in ticks for d in t):
            if tid in facts["with_prefs"]:
                if nid and state >= orc.ASSIGNED:
                    placed += 1
                elif err.startswith("no suitable node"):
                    unplaced += 1
        counts += facts["outside_counts"]
        branch += facts["outside_branch"]
    if SEEDS >= 32:
        assert placed and unplaced and counts and branch, (placed, unplaced, counts, branch)


# ------------------------------------------------------------------------------------------------------------------ the host layer
def host_script():
    """Two task groups (a SpecVersion each) and 30 one-off tasks with preferences, all constrained to the pool, on 4 200 nodes."""
    ev = pool_nodes(mem_gib=lambda i: 1 + i % 3)
    for sname in ("svcA", "svcB", "svcC"):
        ev.append(("set_service", sname))
    con = ["node.labels.pool==a"]
    for i in range(70):
        ev.append(("create_task", sc.pending(f"a{i:03d}", "svcA", 1, Spec={"Placement": {"Preferences": spread("node.labels.zone"), "Constraints": con},
                                                                         "Resources": {"Reservations": {"MemoryBytes": 600 * MIB}}})))
    for i in range(50):
        ev.append(("create_task", sc.pending(f"b{i:03d}", "svcB", 2, Spec={"Placement": {"Constraints": con, "MaxReplicas": 2}})))
    for j in range(8):   # svcC runs outside the pool already, in one zone
        ev.append(("create_task", running("rc%d" % j, "svcC", "n%05d" % (5 + 70 * j))))
    for i in range(30):
        ev.append(("create_task", sc.pending(f"c{i:03d}", "svcC", Spec={"Placement": {"Preferences": spread("node.labels.zone"), "Constraints": con}})))
    return ev + [("tick",), ("tick",)]


def test_host_layer_keeps_spread_one_offs_in_the_run(monkeypatch):
    monkeypatch.setenv("SWP_HOST", "cxx")
    monkeypatch.setenv("SWP_SCHED_ONEOFF_SPREAD", "1")
    ev = host_script()
    want_ticks, want_rows = oracle_of("compact_host", ev)
    s, k = swhost.HostScheduler(), 0
    for x in ev:
        if x[0] == "tick":
            b0 = s.e.stats()["batches"]
            got = sorted(key(d) for d in s.tick())
            assert got == want_ticks[k], (k, [(a, b) for a, b in zip(want_ticks[k], got) if a != b][:5])
            if k == 0:
                st = s.e.stats()   # the call for the two task groups, then ONE batch with a spread segment over the 30 tasks
                assert st["batches"] == b0 + 2 and st["scan_tasks"] == 30 and st["scan_launches"] == 1, st
            k += 1
        else:
            getattr(s, x[0])(*x[1:])
    for nid, a in want_rows.items():
        b = s.node_info(nid)
        assert a["ActiveTasksCount"] == b["ActiveTasksCount"] and a["AvailableResources"]["MemoryBytes"] == b["AvailableResources"]["MemoryBytes"], nid


def test_without_the_knob_the_host_layer_splits_as_before(monkeypatch):
    monkeypatch.setenv("SWP_HOST", "cxx")
    ev = host_script()
    want_ticks, _ = oracle_of("compact_host", ev)
    s = swhost.HostScheduler()
    for x in ev[:-1]:
        if x[0] == "tick":
            assert sorted(key(d) for d in s.tick()) == want_ticks[0]
            assert s.e.stats()["batches"] == 31   # (the two task groups in one call; every one-off task has preferences: 30 calls for groups of one)
        else:
            getattr(s, x[0])(*x[1:])
