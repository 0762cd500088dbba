"""GPU parity of k_waterfill (csrc/swp_waterfill.hpp): runs of identical one-off tasks placed by water-filling over
(failure class, svcCount, ActiveTasksCount, node index) instead of task by task must give the oracle's placements bit for bit —
node order inside a level, nodes that fill up in the middle of a run, MaxReplicas, runs that end in "no suitable node", batches
that mix runs with single tasks (host ports keep a task out of a run)."""
import os
import random

import numpy as np
import pytest

import orc
import parity_util as pu
from swarmkit_amd import host as swhost
from swarmkit_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture
def waterfill_env():
    old = os.environ.get("SWP_WATERFILL")
    yield
    if old is None:
        os.environ.pop("SWP_WATERFILL", None)
    else:
        os.environ["SWP_WATERFILL"] = old


def run_both(wl, mode):
    op, oe, _ = pu.oracle_run(wl)
    os.environ["SWP_WATERFILL"] = mode
    ep, ee, s, *_ = pu.engine_run(wl)
    pu.assert_same(op, oe, ep, ee)
    return s.e.stats()["waterfill_tasks"]


@pytest.mark.parametrize("name,T,N,services", [("cfg3", 3000, 300, 40), ("cfg3", 3000, 300, 3), ("cfg3", 2500, 700, 1), ("cfg4", 3000, 700, 25),
                                               ("cfg2", 3000, 50, 6), ("cfg1", 500, 40, 1), ("cfg4", 4000, 200, 1)])
def test_service_major_runs(waterfill_env, name, T, N, services):
    wl = synth.Workload(name, T=T, N=N, services=services, order="major")
    assert run_both(wl, "1") > T // 2   # the runs really went through k_waterfill


def test_round_robin_order_has_no_runs_and_still_agrees(waterfill_env):
    wl = synth.Workload("cfg3", T=2000, N=300)
    assert run_both(wl, "1") == 0


@pytest.mark.parametrize("N", [1, 63, 65, 1025, 5000, 20000])
def test_node_counts(waterfill_env, N):
    """one node per thread, several per thread, fewer nodes than threads; up to 20 000 nodes"""
    wl = synth.Workload("cfg3", T=1500, N=N, services=4, order="major")
    run_both(wl, "1")


def test_default_policy_takes_the_reference_benchmark_shape(waterfill_env):
    """Without the knob: a batch that is one long run (the reference's benchScheduler: every task of ONE service) is water-filled."""
    wl = synth.Workload("cfg2", T=5000, N=120, services=1, order="major")
    os.environ.pop("SWP_WATERFILL", None)
    op, oe, _ = pu.oracle_run(wl)
    ep, ee, s, *_ = pu.engine_run(wl)
    pu.assert_same(op, oe, ep, ee)
    assert s.e.stats()["waterfill_tasks"] == wl.T


def test_off_switch(waterfill_env):
    wl = synth.Workload("cfg3", T=1500, N=200, services=2, order="major")
    assert run_both(wl, "0") == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# Runs placed from REAL cluster states: the same event script through the oracle and through the host layer, SWP_WATERFILL=1, tasks
# created service-major (no host ports, generic reservations or mounts: every service's stretch of a tick is a run). Every tick is compared
# decision for decision (node, state, Err string), the node rows afterwards; stats()["waterfill_tasks"] must show that at least half of the
# tasks of the ticks under test went through k_waterfill.
GIB = 1 << 30
CPU = 10**9


@pytest.fixture
def forced(waterfill_env):
    os.environ["SWP_WATERFILL"] = "1"


def node_doc(i, cpus=4, gib=16, version=None):
    d = {"ID": "n%05d" % i, "Spec": {"Annotations": {"Name": "node%d" % i}, "Availability": 0}, "Status": {"State": orc.READY, "Addr": "10.0.%d.%d" % (i >> 8, i & 255)},
         "Description": {"Hostname": "h%d" % i, "Resources": {"NanoCPUs": cpus * CPU, "MemoryBytes": gib * GIB}}}
    if version is not None:
        d["Meta"] = {"Version": {"Index": version}}
    return d


def reservations(cpu=0, mem=0):
    return {"Resources": {"Reservations": {"NanoCPUs": cpu, "MemoryBytes": mem}}}


class Both:
    """One event script into the oracle and into the engine's host layer."""

    def __init__(self, n_nodes, cpus=4, gib=16, versions=False):
        self.o, self.e = orc.Oracle(), swhost.HostScheduler()
        self.N = n_nodes
        self.nodes = {}
        for i in range(n_nodes):
            self.node(node_doc(i, cpus, gib, 10 + i if versions else None))
        self.services, self.docs, self.placed, self.seq = {}, {}, {}, 0
        self.wf0 = self.waterfilled()

    def both(self, name, *args):
        return [getattr(s, name)(*args) for s in (self.o, self.e)]

    def node(self, doc):
        self.nodes[doc["ID"]] = doc
        self.both("create_node", doc)

    def service(self, name, spec=None):
        """A one-off service (its tasks carry no SpecVersion): Spec is the tasks' Spec."""
        self.services[name] = spec
        self.both("set_service", name)

    def add(self, name, count):
        """`count` new pending tasks of one service, next to each other in the queue (ids ascend in creation order)."""
        ids = []
        for _ in range(count):
            t = {"ID": "t%07d" % self.seq, "ServiceID": name, "DesiredState": orc.RUNNING, "Status": {"State": orc.PENDING}}
            if self.services[name]:
                t["Spec"] = self.services[name]
            self.seq += 1
            self.docs[t["ID"]] = t
            self.both("create_task", t)
            ids.append(t["ID"])
        return ids

    def fail_on(self, name, node_id, times, spec_version=None):
        """`times` recorded failures of the service on the node, as the reference's faulty-node scenario makes them: a task that runs there is
        reported FAILED (updateTask -> NodeInfo.taskFailed)."""
        for _ in range(times):
            t = {"ID": "f%07d" % self.seq, "ServiceID": name, "NodeID": node_id, "DesiredState": orc.RUNNING, "Status": {"State": orc.RUNNING}}
            if spec_version is not None:
                t["SpecVersion"] = {"Index": spec_version}
            self.seq += 1
            self.both("create_task", t)
            self.both("update_task", dict(t, Status={"State": orc.FAILED}))

    def delete(self, tid):
        self.both("delete_task", dict(self.docs[tid], NodeID=self.placed.pop(tid), Status={"State": orc.RUNNING}))

    def waterfilled(self):
        return self.e.e.stats()["waterfill_tasks"]

    def tick(self, floor=True):
        """One tick of both; returns {task: (node, Err)}. floor: at least half of the tick's tasks went through k_waterfill."""
        before = self.waterfilled()
        do = sorted((d["ID"], d["NodeID"], d["Err"], d["State"]) for d in self.o.tick())
        de = sorted((d["ID"], d["NodeID"], d["Err"], d["State"]) for d in self.e.tick())
        assert do == de, [(a, b) for a, b in zip(do, de) if a != b][:5]
        for tid, nid, err, st in do:
            if nid and st >= orc.ASSIGNED:
                self.placed[tid] = nid
        if floor:
            assert 2 * (self.waterfilled() - before) >= len(do), (self.waterfilled() - before, len(do))
        return {tid: (nid if st >= orc.ASSIGNED else "", err) for tid, nid, err, st in do}

    def same_nodes(self):
        for nid in self.nodes:
            a, b = self.o.node_info(nid), self.e.node_info(nid)
            assert a["ActiveTasksCount"] == b["ActiveTasksCount"], nid
            assert a["AvailableResources"]["NanoCPUs"] == b["AvailableResources"]["NanoCPUs"], nid
            assert a["AvailableResources"]["MemoryBytes"] == b["AvailableResources"]["MemoryBytes"], nid
            nz = lambda m: {k: v for k, v in m.items() if v}   # noqa: E731 (the Go map keeps a key whose count went back to 0)
            assert nz(a["ActiveTasksCountByService"]) == nz(b["ActiveTasksCountByService"]), nid
            assert sorted(a["Tasks"]) == sorted(b["Tasks"]), nid


def on(decisions, ids):
    """How many of the tasks `ids` each node got."""
    c = {}
    for t in ids:
        if decisions[t][0]:
            c[decisions[t][0]] = c.get(decisions[t][0], 0) + 1
    return c


@pytest.mark.parametrize("N", [63, 1025])
def test_second_and_third_ticks(forced, N):
    """The same services get more tasks after an earlier tick placed some of them and tasks of OTHER services: non-empty exception lists,
    uneven task counts. Tasks are deleted in between, so entries drop to 0 and those nodes rejoin the clean set."""
    b = Both(N)
    b.service("svcA", reservations(CPU // 4, GIB // 4))
    b.service("svcB", reservations(CPU // 2, 0))
    b.service("svcC")
    a1 = b.add("svcA", N // 2 + 7)
    b1 = b.add("svcB", N // 3 + 2)
    b.add("svcC", 5)
    b.tick()
    b.same_nodes()
    for t in a1[::3] + b1[::2]:
        b.delete(t)
    a2 = b.add("svcA", N + N // 2)
    b.add("svcB", N // 3)
    b.tick()
    b.same_nodes()
    for t in a2[::5]:
        b.delete(t)
    b.add("svcC", N // 4 + 2)
    b.add("svcA", N)
    b.tick()
    b.same_nodes()


def test_failure_classes(forced):
    """Recorded failures below, at and above MAX_FAILURES (5), and failures of ANOTHER spec version, which must not count: the run fills the
    class-0 nodes (4 tasks each: 4 cpus, 1 a task) before the node with 5 failures, and that one before the node with 8."""
    b = Both(65)
    b.service("svcA", reservations(CPU, 0))
    b.fail_on("svcA", "n00001", 3)
    b.fail_on("svcA", "n00002", 5)
    b.fail_on("svcA", "n00003", 8)
    b.fail_on("svcA", "n00004", 6, spec_version=7)
    ids = b.add("svcA", 63 * 4 + 6)
    got = on(b.tick(), ids)
    b.same_nodes()
    assert got["n00000"] == 4 and got["n00001"] == 4 and got["n00004"] == 4   # 3 failures: class 0; another version: not this service's
    assert got["n00002"] == 4 and got["n00003"] == 2
    ids = b.add("svcA", 5)   # the second tick meets the entries the first left: 2 places on the node with 8 failures, then no node
    dec = b.tick()
    assert on(dec, ids) == {"n00003": 2}
    assert sum(1 for t in ids if not dec[t][0]) == 3
    b.same_nodes()


def test_maxreplicas_against_earlier_replicas(forced):
    """Tick 1 places up to the limit on some nodes; tick 2's run skips exactly those and ends in the oracle's MaxReplicas tail."""
    b = Both(63)
    b.service("svcA", {"Placement": {"MaxReplicas": 2}})
    b.service("svcB")
    first = b.add("svcA", 80)   # 63 nodes get one, 17 of them a second
    b.add("svcB", 10)
    full = {n for n, k in on(b.tick(), first).items() if k == 2}
    assert len(full) == 17
    ids = b.add("svcA", 60)
    dec = b.tick()
    got = on(dec, ids)
    assert len(got) == 46 and not (set(got) & full) and set(got.values()) == {1}
    tail = [dec[t][1] for t in ids if not dec[t][0]]
    assert len(tail) == 14 and set(tail) == {"no suitable node (max replicas per node limit exceed)"}
    b.same_nodes()


def test_over_committed_nodes(forced):
    """A node's resources are updated downwards below what runs there: its cpu residual is negative. A run whose reservation names memory
    alone must avoid it (ResourceFilter.Check compares the reservation of 0 with the negative residual, filter.go:78); a run without
    Resources uses it; and so does a run whose Reservations are present and all 0, because ResourceFilter.SetTask switches the filter off
    for it (filter.go:68) — the oracle decides, the asserts below only name what it says."""
    b = Both(65)
    b.service("svcB", reservations(CPU, 0))
    b.service("svcMem", reservations(0, GIB // 4))
    b.service("svcZero", reservations(0, 0))
    b.service("svcNone")
    b.add("svcB", 130)   # two a node
    b.tick()
    b.node(node_doc(7, cpus=1))   # 1 cpu against 2 reserved
    assert b.o.node_info("n00007")["AvailableResources"]["NanoCPUs"] == -CPU
    mem, zero, none = b.add("svcMem", 130), b.add("svcZero", 130), b.add("svcNone", 130)
    dec = b.tick()
    assert "n00007" not in on(dec, mem) and len(on(dec, mem)) == 64
    assert on(dec, none)["n00007"] >= 2
    assert on(dec, zero)["n00007"] >= 2
    b.same_nodes()


def test_rejected_decisions_of_a_waterfilled_tick(forced):
    """test_engine_rollback's rejected-decision script with the placements coming out of k_waterfill: the store refuses every third one,
    the next tick (the refused tasks and new runs) must match the oracle."""
    b = Both(300)
    b.service("svcA", reservations(CPU // 4, GIB // 8))
    b.service("svcB", {"Placement": {"MaxReplicas": 3}})
    b.add("svcA", 1400)
    b.add("svcB", 1100)
    dec = b.tick()
    b.same_nodes()
    placed = sorted(t for t in dec if dec[t][0])
    assert len(placed) > 2000
    rejected = placed[::3]
    for tid in rejected:
        assert b.e.reject_decision(tid) is True
        b.o.delete_task(dict(b.docs[tid], NodeID=dec[tid][0], Status={"State": orc.ASSIGNED}))
        b.o.create_task(b.docs[tid])
        del b.placed[tid]
    assert b.e.reject_decision(rejected[0]) is False
    b.same_nodes()
    b.add("svcA", 300)
    b.add("svcB", 200)
    again = b.tick()
    assert set(rejected) <= set(again)
    b.same_nodes()


def test_a_stale_node_version_after_a_waterfilled_tick(forced):
    """test_engine_rollback's stale-node-version script over water-filled placements: two nodes moved in the store between the tick and
    the commit, their whole groups are handed back (reject_node walks the per-node chains k_waterfill wrote)."""
    b = Both(120, versions=True)
    b.service("svcA", reservations(CPU // 8, 0))
    b.service("svcB")
    b.add("svcA", 1200)
    b.add("svcB", 800)
    dec = b.tick()
    plan = b.e.commit_plan()
    moved = [plan["Nodes"][3], plan["Nodes"][17]]
    for g in moved:
        assert b.e.reject_node(g["NodeID"]) == len(g["Tasks"])
        for tid in g["Tasks"]:
            b.o.delete_task(dict(b.docs[tid], NodeID=dec[tid][0], Status={"State": orc.ASSIGNED}))
            b.o.create_task(b.docs[tid])
            del b.placed[tid]
    for g in moved:
        i = int(g["NodeID"][1:])
        b.node(node_doc(i, version=11 + i))
    b.same_nodes()
    b.add("svcA", 200)
    again = b.tick()
    assert {t for g in moved for t in g["Tasks"]} <= set(again)
    b.same_nodes()


@pytest.mark.parametrize("N", [65, 1023])
def test_runs_between_block_resolver_stretches_with_prior_state(forced, N):
    """Two ticks, both mixing runs with single tasks (a service with one task is no run: the block resolver decides the stretch and
    rebuilds its state from what the runs left, and the other way round)."""
    b = Both(N)
    b.service("svcA", reservations(CPU // 4, 0))
    b.service("svcB", {"Placement": {"MaxReplicas": 2}})
    for k in range(40):
        b.service("one%02d" % k, reservations(CPU // 8, GIB // 8) if k % 2 else None)
    for tick in range(2):
        b.add("svcA", 300)
        for k in range(0, 20):
            b.add("one%02d" % k, 1)
        b.add("svcB", N // 2 + 30)
        for k in range(20, 40):
            b.add("one%02d" % k, 1)
        b.add("svcA", 150)
        b.tick()
        b.same_nodes()
        for t in sorted(b.placed)[::7]:
            b.delete(t)


@pytest.mark.parametrize("seed", range(int(os.environ.get("SWP_FUZZ_FIRST", "0")), int(os.environ.get("SWP_FUZZ_FIRST", "0")) + int(os.environ.get("SWP_FUZZ_SEEDS", "12"))))
def test_seeded_runs_from_cluster_states(forced, seed):
    """All of the above drawn at random: node count, services with reservations / MaxReplicas, recorded failures (also of another spec
    version), the number of ticks, single tasks of one-task services between the runs, deletions and a shrunken node in between, and in
    some seeds a rollback of water-filled placements (decisions the store refuses, or a whole node's group). Every tick clears the
    waterfill floor. SWP_FUZZ_SEEDS / SWP_FUZZ_FIRST for a soak."""
    rng = random.Random(0x3A7E4 + seed)
    N = rng.choice([1, 63, 65, 1023, 1025, 2049, 5000])
    b = Both(N, cpus=rng.choice([2, 4, 8]))
    names = []
    for k in range(rng.randrange(2, 6)):
        spec = {}
        if rng.random() < 0.7:
            spec.update(reservations(rng.choice([0, CPU // 4, CPU // 2, CPU]), rng.choice([0, GIB // 4, GIB])))
        if rng.random() < 0.35:
            spec["Placement"] = {"MaxReplicas": rng.choice([1, 2, 4])}
        names.append("svc%d" % k)
        b.service(names[-1], spec or None)
    for k in range(4):   # services that only ever get one task a tick: no run, the block resolver's stretch between two runs
        b.service("one%d" % k, reservations(CPU // 4, 0) if k % 2 else None)
    for _ in range(rng.randrange(0, 5)):
        b.fail_on(rng.choice(names), "n%05d" % rng.randrange(N), rng.choice([1, 4, 5, 6, 9]), spec_version=rng.choice([None, None, 3]))
    budget = 2500
    for tick in range(rng.randrange(2, 5)):
        chosen = rng.sample(names, rng.randrange(1, len(names) + 1))
        for i, name in enumerate(chosen):
            k = min(rng.choice([2, 30, N // 2 + 1, N, N + 3, 2 * N + 1]), 900, max(budget, 2))
            if i == 0:
                k = max(k, 40)   # (left-over single tasks of earlier ticks and the one-task services stay below half of the tick)
            b.add(name, k)
            budget -= k
            if rng.random() < 0.5:
                b.add("one%d" % rng.randrange(4), 1)
        dec = b.tick()
        b.same_nodes()
        act = rng.random()
        if act < 0.25:     # the store refuses some of the decisions (test_engine_rollback.py's script)
            for tid in sorted(t for t in dec if dec[t][0])[::rng.choice([2, 5])]:
                assert b.e.reject_decision(tid) is True
                b.o.delete_task(dict(b.docs[tid], NodeID=dec[tid][0], Status={"State": orc.ASSIGNED}))
                b.o.create_task(b.docs[tid])
                del b.placed[tid]
            b.same_nodes()
        elif act < 0.4:    # ... or a whole node's group (a stale node version)
            plan = b.e.commit_plan()
            if plan["Nodes"]:
                g = rng.choice(plan["Nodes"])
                assert b.e.reject_node(g["NodeID"]) == len(g["Tasks"])
                for tid in g["Tasks"]:
                    b.o.delete_task(dict(b.docs[tid], NodeID=dec[tid][0], Status={"State": orc.ASSIGNED}))
                    b.o.create_task(b.docs[tid])
                    del b.placed[tid]
                b.same_nodes()
        if b.placed:
            for t in rng.sample(sorted(b.placed), len(b.placed) // rng.choice([2, 3, 10])):
                b.delete(t)
        if rng.random() < 0.4:
            b.node(node_doc(rng.randrange(N), cpus=1, gib=1))   # shrunk below what may run there
    b.tick(floor=False)   # what the last step handed back or left pending: decided again, whatever its shape
    b.same_nodes()


def test_the_scan_resolver_is_kept_from_failure_counts_beyond_its_keys(waterfill_env):
    """A stretch of tasks whose service already runs on every node decides one task a round in the block resolver, which hands it to
    the scan resolver — whose keys hold 255 recorded failures: with 256 on a node the batch used to end in SWP_ERANGE. build_batch now
    marks such a batch and the block resolver decides it alone. With 255 the scan resolver still takes the stretch (the control: the
    script does reach it)."""
    for fails, scanned in ((255, True), (256, False)):
        os.environ["SWP_WATERFILL"] = "0"
        b = Both(5, cpus=64)
        b.service("svcA")
        b.fail_on("svcA", "n00001", fails)
        b.add("svcA", 10)
        b.tick(floor=False)
        ids = b.add("svcA", 600)
        got = on(b.tick(floor=False), ids)
        assert (b.e.e.stats()["scan_tasks"] > 0) == scanned, (fails, b.e.e.stats()["scan_tasks"])
        assert got["n00000"] == 150 and "n00001" not in got
        b.same_nodes()


def test_failure_counts_beyond_the_packed_class(forced):
    """One service has 258 recorded failures on one node (failure class 254, the last one k_waterfill's packed key holds) and 259 on
    another (class 255, beyond it). The reference only ranks such nodes last: clean node first, then 258, then 259. k_waterfill would give
    the 259 node capacity 0 (tests/test_emu_waterfill.py records that), so build_batch hands a run of such a service to the block resolver;
    the other service's run of the same tick is water-filled."""
    b = Both(3)
    b.service("svcA", reservations(CPU, 0))
    b.service("svcB")
    b.fail_on("svcA", "n00001", 258)
    b.fail_on("svcA", "n00002", 259)
    a, other = b.add("svcA", 10), b.add("svcB", 40)
    before = b.waterfilled()
    dec = b.tick()
    assert on(dec, a) == {"n00000": 4, "n00001": 4, "n00002": 2}
    assert b.waterfilled() - before == len(other)   # svcA's run went to the block resolver
    b.same_nodes()
    a2 = b.add("svcA", 4)    # ... and with the entries of the first tick in the list
    b.add("svcB", 40)
    dec = b.tick()
    assert on(dec, a2) == {"n00002": 2} and sum(1 for t in a2 if not dec[t][0]) == 2
    b.same_nodes()
