"""GPU: swp_enforce_generic (k_enforce for the nodes without a generic task, k_enforce_generic — one wave per node — for the others)
against the oracle's rejectNoncompliantTasks, orc.enforce, node by node. First the struct ABI directly (Engine.enforce_generic: the
records and the four parallel arrays built here from the same docs the oracle reads), then seeded random clusters with irregular
lists through the host layer (swp_sched_enforce -> one swp_enforce_generic call), on one engine and on a shard set of 3."""
import os
import random

import numpy as np
import pytest

import orc
from swarmkit_amd import abi, host as swhost, sched as swsched

pytestmark = pytest.mark.gpu

BIG = 10**10


def node_doc(nid, generic, labels=None, cpu=BIG, mem=BIG):
    return {"ID": nid, "Spec": {"Annotations": {"Labels": labels or {}}, "Availability": 0}, "Status": {"State": orc.READY},
            "Description": {"Resources": {"NanoCPUs": cpu, "MemoryBytes": mem, "Generic": generic}}}


def task_doc(tid, nid, gen=None, cons=None, rsv=None, desired=orc.RUNNING, state=orc.RUNNING):
    t = {"ID": tid, "NodeID": nid, "DesiredState": desired, "Status": {"State": state}, "Spec": {}}
    if gen is not None:
        t["AssignedGenericResources"] = gen
    if cons:
        t["Spec"]["Placement"] = {"Constraints": cons}
    if rsv:
        t["Spec"]["Resources"] = {"Reservations": {"NanoCPUs": rsv[0], "MemoryBytes": rsv[1]}}
    return t


def D(kind, value):
    return {"Discrete": {"Kind": kind, "Value": value}}


def N(kind, value):
    return {"Named": {"Kind": kind, "Value": value}}


class Case:
    """One engine with the nodes in its mirror (without their generic lists: the sweep reads Description.Resources from the records,
    and the mirror's counts stop at 2^31) and the request as records + parallel arrays."""

    def __init__(self, nodes, tasks, **engine_kw):
        self.s = swsched.Scheduler(**engine_kw)
        self.node_docs, self.task_docs = nodes, tasks
        names = {}

        def res(lst):
            out = []
            for x in lst or []:
                (ty, spec), = x.items()
                named = ty == "Named"
                out.append((self.s.e.intern(abi.SPACE_GENERIC_KIND, spec["Kind"]), int(named), names.setdefault(spec["Value"], len(names)) if named else spec["Value"]))
            return out

        nrec, trec, nres, tres, noff, toff, self.owner = [], [], [], [], [0], [0], []
        for nd in nodes:
            bare = dict(nd, Description={"Resources": {k: v for k, v in nd["Description"]["Resources"].items() if k != "Generic"}})
            self.s.create_node(bare)
            mine = sorted((t for t in tasks if t["NodeID"] == nd["ID"]), key=lambda t: t["ID"])
            r = nd["Description"]["Resources"]
            nrec.append((self.s.e.intern(abi.SPACE_NODE_ID, nd["ID"]), len(trec), len(mine), 0, r["NanoCPUs"], r["MemoryBytes"]))
            nres += res(r.get("Generic"))
            noff.append(len(nres))
            for t in mine:
                rsv = t["Spec"].get("Resources", {}).get("Reservations")
                cons = t["Spec"].get("Placement", {}).get("Constraints")
                trec.append((rsv["NanoCPUs"] if rsv else 0, rsv["MemoryBytes"] if rsv else 0, self.s.constraint_set(cons) if cons else 0,
                             abi.ENF_RESERVATIONS if rsv else 0, t["DesiredState"], t["Status"]["State"]))
                tres += res(t.get("AssignedGenericResources"))
                toff.append(len(tres))
                self.owner.append((nd["ID"], t["ID"]))
        self.nodes = np.array(nrec, dtype=abi.ENF_NODE_DTYPE)
        self.tasks = np.array(trec, dtype=abi.ENF_TASK_DTYPE)
        self.nres = np.array(nres, dtype=abi.ENF_RES_DTYPE)
        self.tres = np.array(tres, dtype=abi.ENF_RES_DTYPE)
        self.noff = np.array(noff, dtype=np.uint32)
        self.toff = np.array(toff, dtype=np.uint32)

    def named(self, rej):
        out = {nd["ID"]: [] for nd in self.node_docs}
        for (nid, tid), r in zip(self.owner, rej):
            assert r in (0, 1)
            if r:
                out[nid].append(tid)
        return out

    def run(self):
        return self.named(self.s.e.enforce_generic(self.nodes, self.tasks, self.noff, self.nres, self.toff, self.tres))

    def oracle(self):
        return {nd["ID"]: orc.enforce(nd, sorted((t for t in self.task_docs if t["NodeID"] == nd["ID"]), key=lambda t: t["ID"]), {}) for nd in self.node_docs}


def six_tasks(nid="id0"):
    """The scenario of test_engine_enforcer's test_generic_resources_the_loop_ends_at_the_first_missing_assignment."""
    node = node_doc(nid, [D("gpu", 2), N("fpga", "f0")], {"zone": "a"})
    tasks = [task_doc("t0", nid, [D("gpu", 1)]), task_doc("t1", nid, [N("fpga", "f0")]), task_doc("t2", nid, None, ["node.labels.zone==b"]),
             task_doc("t3", nid, [D("gpu", 2)]), task_doc("t4", nid, None, ["node.labels.zone==b"]), task_doc("t5", nid, [N("fpga", "f0")])]
    return node, tasks


def test_the_loop_ends_at_the_first_missing_assignment():
    node, tasks = six_tasks()
    c = Case([node], tasks)
    want = c.oracle()
    assert want == {"id0": ["t2", "t3"]}   # t2: constraint; t3: one gpu left, two assigned -> rejected, the loop ends: t4 (constraint) and t5 (fpga gone) stay
    assert c.run() == want


def test_a_break_stays_inside_its_node():
    """Three nodes, only the middle one with assignments: its break ends its own walk; the neighbours (k_enforce's share of the call)
    reject by constraint and by reservation as swp_enforce would."""
    left = node_doc("id-a", [D("gpu", 1)], {"zone": "a"}, cpu=10**9, mem=10**9)
    mid, mid_tasks = six_tasks("id-b")
    right = node_doc("id-c", [], {"zone": "b"}, cpu=10**9, mem=10**9)
    tasks = [task_doc("a0", "id-a", None, ["node.labels.zone==b"]), task_doc("a1", "id-a", None, None, (6 * 10**8, 1)), task_doc("a2", "id-a", None, None, (6 * 10**8, 1)),
             task_doc("a3", "id-a", [], None, (10**8, 1))] + mid_tasks + \
            [task_doc("c0", "id-c", None, ["node.labels.zone==b"]), task_doc("c1", "id-c", None, ["node.labels.zone==a"]), task_doc("c2", "id-c", None, None, (1, 2 * 10**9))]
    c = Case([left, mid, right], tasks)
    want = c.oracle()
    assert want == {"id-a": ["a0", "a2"], "id-b": ["t2", "t3"], "id-c": ["c1", "c2"]}
    assert c.run() == want


def test_the_decisive_entry_lies_behind_the_chunk_border():
    """70 Named entries; the tasks hold numbers 66, 3, again 66 (gone: break) — and before that a name the list ends without."""
    lst = [N("gpu", "g%02d" % i) for i in range(70)]
    tasks = [task_doc("t0", "id0", [N("gpu", "g65")]), task_doc("t1", "id0", [N("gpu", "g02")]), task_doc("t2", "id0", [N("gpu", "g69"), N("gpu", "g00")]),
             task_doc("t3", "id0", [N("gpu", "g65")]), task_doc("t4", "id0", None, ["node.labels.zone==b"])]
    c = Case([node_doc("id0", lst)], tasks)
    want = c.oracle()
    assert want == {"id0": ["t3"]}
    assert c.run() == want
    c2 = Case([node_doc("id0", lst)], [task_doc("t0", "id0", [N("gpu", "g65")]), task_doc("t1", "id0", [N("gpu", "nope")]), task_doc("t2", "id0", None, ["node.labels.zone==b"])])
    assert c2.oracle() == {"id0": ["t1"]}
    assert c2.run() == c2.oracle()


def test_a_kind_listed_twice():
    """Discrete 2, Discrete 1: HasResource reads the first entry, ConsumeNodeResources subtracts from both."""
    tasks = [task_doc("t%d" % i, "id0", [D("gpu", 1)]) for i in range(4)]
    c = Case([node_doc("id0", [D("gpu", 2), D("gpu", 1)])], tasks)
    want = c.oracle()
    assert want == {"id0": ["t2"]}   # after two claims {} is left of both entries
    assert c.run() == want


def test_discrete_then_named_under_one_kind():
    """The Discrete entry in front decides: a Named assignment is gone at once although its name is listed behind it."""
    lst = [D("gpu", 3), N("gpu", "g0")]
    c = Case([node_doc("id0", lst)], [task_doc("t0", "id0", [D("gpu", 1)]), task_doc("t1", "id0", [N("gpu", "g0")]), task_doc("t2", "id0", [D("gpu", 1)])])
    want = c.oracle()
    assert want == {"id0": ["t1"]}
    assert c.run() == want
    # ... and the other way round: Named in front, a Discrete assignment is gone at once
    c = Case([node_doc("id0", lst[::-1])], [task_doc("t0", "id0", [N("gpu", "g0")]), task_doc("t1", "id0", [D("gpu", 1)]), task_doc("t2", "id0", [D("gpu", 9)])])
    want = c.oracle()
    assert want == {"id0": ["t2"]}   # t0 takes the name; then the Discrete entry is the kind's first
    assert c.run() == want


def test_two_discrete_assignments_of_one_kind():
    """Each is checked alone against the entry (2 <= 3 twice), then both subtract: 3 - 2 - 2 <= 0, the entry is gone."""
    tasks = [task_doc("t0", "id0", [D("gpu", 2), D("gpu", 2)]), task_doc("t1", "id0", [D("gpu", 1)]), task_doc("t2", "id0", [D("gpu", 1)])]
    c = Case([node_doc("id0", [D("gpu", 3)])], tasks)
    want = c.oracle()
    assert want == {"id0": ["t1"]}
    assert c.run() == want


def test_a_discrete_value_above_2_31():
    big = 2**31 + 5
    tasks = [task_doc("t0", "id0", [D("gpu", 2**31)]), task_doc("t1", "id0", [D("gpu", 5)]), task_doc("t2", "id0", [D("gpu", 1)])]
    c = Case([node_doc("id0", [D("gpu", big)])], tasks)
    want = c.oracle()
    assert want == {"id0": ["t2"]}   # 2^31 + 5 - 2^31 = 5, - 5 = exactly 0: gone
    assert c.run() == want
    c = Case([node_doc("id0", [D("gpu", big)])], [task_doc("t0", "id0", [D("gpu", big + 1)]), task_doc("t1", "id0", [D("gpu", 1)])])
    assert c.oracle() == {"id0": ["t0"]}
    assert c.run() == c.oracle()


def test_without_assignments_the_answer_is_swp_enforce():
    left = node_doc("id-a", [D("gpu", 1)], {"zone": "a"}, cpu=10**9, mem=10**9)
    tasks = [task_doc("a0", "id-a", None, ["node.labels.zone==b"]), task_doc("a1", "id-a", None, None, (6 * 10**8, 1)), task_doc("a2", "id-a", None, None, (6 * 10**8, 1)),
             task_doc("a3", "id-a", None, None, (1, 1), desired=orc.SHUTDOWN), task_doc("a4", "id-a", None, None, (1, 1), state=orc.FAILED)]
    c = Case([left], tasks)
    zeros = np.zeros(len(c.tasks) + 1, dtype=np.uint32)
    got = c.s.e.enforce_generic(c.nodes, c.tasks, c.noff, c.nres, zeros, c.tres)
    assert list(got) == list(c.s.e.enforce(c.nodes, c.tasks))
    assert c.named(got) == c.oracle() == {"id-a": ["a0", "a2"]}


def test_refusals_leave_the_verdicts_untouched():
    node, tasks = six_tasks()
    c = Case([node], tasks)
    kind = c.s.e.intern(abi.SPACE_GENERIC_KIND, "gpu")

    def refused(noff=None, nres=None, toff=None, tres=None, nodes=None):
        out = np.full(len(c.tasks), 7, dtype=np.uint8)
        with pytest.raises(abi.SwpError) as err:
            c.s.e.enforce_generic(c.nodes if nodes is None else nodes, c.tasks, c.noff if noff is None else noff, c.nres if nres is None else nres,
                                  c.toff if toff is None else toff, c.tres if tres is None else tres, out=out)
        assert list(out) == [7] * len(c.tasks)
        return err.value.code

    down = c.toff.copy()
    down[2], down[3] = down[3], down[1]
    assert refused(toff=down) == abi.SWP_EINVAL                     # a non-monotone offset
    unknown = c.nres.copy()
    unknown["kind"][0] = kind + 1000
    assert refused(nres=unknown) == abi.SWP_EINVAL                  # an unknown kind
    two = c.tres.copy()
    two["named"][1] = 2
    assert refused(tres=two) == abi.SWP_EINVAL                      # named = 2
    absent = c.nodes.copy()
    absent["node"][0] = 12345
    assert refused(nodes=absent) == abi.SWP_ENOTFOUND               # as swp_enforce
    assert c.run() == c.oracle()                                    # ... and the engine is as it was


# ---- seeded random clusters through the host layer ----
STATES = [orc.NEW, orc.PENDING, orc.ASSIGNED, orc.READY_T, orc.RUNNING, orc.RUNNING, orc.RUNNING, orc.COMPLETE, orc.SHUTDOWN, orc.FAILED]
CONS = ["node.labels.zone==a", "node.labels.zone!=b", "node.role==manager", "node.hostname==h3", "bogus expr"]
KINDS = ["gpu", "fpga", "tpu"]


def _entry(rng, kind=None, names=4):
    kind = kind or rng.choice(KINDS)
    if rng.random() < 0.5:
        return N(kind, "%s%d" % (kind[0], rng.randrange(names)))
    return D(kind, rng.randrange(0, 5))


def cluster(seed):
    rng = random.Random(0x6E4F + seed)
    nodes, tasks = [], []
    for i in range([1, 5, 70, 300][seed % 4]):   # (every size within any four seeds in a row)
        labels = {"zone": rng.choice("abc")} if rng.random() < 0.8 else {}
        d = {"ID": "n%05d" % i, "Role": rng.choice(["WORKER", "WORKER", "MANAGER"]), "Spec": {"Annotations": {"Name": "x%d" % i, "Labels": labels}, "Availability": rng.choice([0, 0, 0, 0, 1, 2])},
             "Status": {"State": orc.READY}}
        lst = []
        if rng.random() < 0.9:
            d["Description"] = {"Hostname": "h%d" % i, "Resources": {"NanoCPUs": rng.choice([0, 1, 2, 4]) * 10**9, "MemoryBytes": rng.choice([0, 1, 4, 8]) << 30}}
            if rng.random() < 0.8:   # irregular on purpose: kinds twice, both types under one kind, now and then more than a wave holds
                long_list = rng.random() < 0.08
                lst = [_entry(rng, names=80 if long_list else 4) for _ in range(rng.randrange(65, 100) if long_list else rng.randrange(0, 7))]
                d["Description"]["Resources"]["Generic"] = lst
        nodes.append(d)
        for j in range(rng.randrange(0, 10)):
            t = {"ID": "t%05d-%02d" % (i, rng.randrange(60)), "NodeID": d["ID"], "ServiceID": "s%d" % rng.randrange(6), "DesiredState": rng.choice(STATES), "Status": {"State": rng.choice(STATES)}, "Spec": {}}
            if rng.random() < 0.5:
                t["Spec"]["Resources"] = {"Reservations": {"NanoCPUs": rng.choice([0, 5, 10, 20]) * 10**8, "MemoryBytes": rng.choice([0, 256, 1024, 3000]) << 20}}
            if rng.random() < 0.3:
                t["Spec"]["Placement"] = {"Constraints": rng.sample(CONS, rng.randrange(0, 3))}
            if rng.random() < 0.4:
                a = []
                for _ in range(rng.randrange(0, 4)):
                    x = _entry(rng)
                    if lst and rng.random() < 0.7:
                        x = {k: dict(v) for k, v in rng.choice(lst).items()}
                        if "Discrete" in x and x["Discrete"]["Value"] > 1:
                            x["Discrete"]["Value"] = rng.randrange(1, x["Discrete"]["Value"] + 1)
                    if a and rng.random() < 0.25:
                        x = _entry(rng, kind=list(a[-1].values())[0]["Kind"])
                    a.append(x)
                t["AssignedGenericResources"] = a
            tasks.append(t)
    tasks = list({t["ID"]: t for t in tasks}.values())
    services = {}
    for k in range(rng.randrange(0, 5)):
        pl = {"Constraints": rng.sample(CONS, rng.randrange(0, 3))} if rng.random() < 0.7 else None
        services["s%d" % k] = {"ID": "s%d" % k, "Spec": {"Task": ({"Placement": pl} if pl is not None else {})}}
    return nodes, tasks, services


_oracle_cache = {}


def oracle_of(seed):
    """The oracle's answer for a seed, computed once for the single engine and the shard set."""
    if seed not in _oracle_cache:
        nodes, tasks, services = cluster(seed)
        _oracle_cache[seed] = {nd["ID"]: orc.enforce(nd, sorted((t for t in tasks if t["NodeID"] == nd["ID"]), key=lambda t: t["ID"]), services)
                               for nd in nodes if nd["Spec"]["Availability"] == 0}
    return _oracle_cache[seed]


def host_enforce(seed, **engine_kw):
    nodes, tasks, services = cluster(seed)
    s = swhost.HostScheduler(**engine_kw)
    for nd in nodes:
        s.create_node(nd)
    tbn = {}
    for t in tasks:
        tbn.setdefault(t["NodeID"], []).append(t)
    return swhost.enforce(s, nodes, tbn, services)


SEEDS = range(int(os.environ.get("SWP_FUZZ_FIRST", "0")), int(os.environ.get("SWP_FUZZ_FIRST", "0")) + int(os.environ.get("SWP_FUZZ_SEEDS", "12")))


@pytest.mark.parametrize("seed", SEEDS)
def test_random_clusters(seed):
    assert host_enforce(seed) == oracle_of(seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_random_clusters_over_a_shard_set(seed):
    assert host_enforce(seed, shards=3, nodes_per_shard=100) == oracle_of(seed)
