"""CPU: processPreassignedTasks through swp_fit_pairs (one engine call per run of pending tasks) against the per-task path (one
swp_check_node + swp_commit per task). Both host layers are the product's C++ one (swarmkit_amd/csrc/swp_sched.cpp) over the engine
double: the plain double's library has no swp_fit_pairs (the weak reference stays null: the per-task path), the second library adds
tests/fake_fit.cpp, the call composed of the double's own check and commit. The double's verdicts are pseudo-random in call order, so
equal decisions mean the batched path judged the same tasks in the same order and booked what the per-task path books."""
import random

import pytest

import fakefit
import fakelib
import orc
from swarmkit_amd import abi, sched as swsched


class FitPair:
    """The same events into a host layer over each library; every answer compared."""

    def __init__(self):
        self.plain = swsched.Scheduler(engine=abi.Engine(lib_path=fakelib.build()))
        self.fitlib = fakefit.build()
        self.fit = swsched.Scheduler(engine=abi.Engine(lib_path=self.fitlib))
        self.steps = 0

    def both(self, name, *args):
        self.steps += 1
        res = []
        for s in (self.plain, self.fit):
            try:
                res.append(("ok", getattr(s, name)(*args)))
            except abi.Unsupported:
                res.append(("unsupported", None))
        assert res[0] == res[1], (self.steps, name, args[:1], res)
        return res[0][1]

    def calls(self):
        return fakefit.fit_calls(self.fitlib)


def _node(i, generic=None):
    d = {"ID": "n%03d" % i, "Status": {"State": 2}, "Spec": {"Availability": 0},
         "Description": {"Hostname": "h%d" % i, "Resources": {"NanoCPUs": 8 * 10**9, "MemoryBytes": 16 << 30}}}
    if generic is not None:
        d["Description"]["Resources"]["Generic"] = generic
    return d


def _task(tid, sid, node, **kw):
    t = {"ID": tid, "ServiceID": sid, "DesiredState": orc.RUNNING, "Status": {"State": orc.PENDING}, "NodeID": node,
         "Spec": {"Resources": {"Reservations": {"NanoCPUs": 10**9, "MemoryBytes": 1 << 30}}}}
    t.update(kw)
    return t


def _mounts():
    return {"Container": {"Mounts": [{"Type": 4, "Source": "group:g", "Target": "/data"}]},
            "Resources": {"Reservations": {"NanoCPUs": 10**9}}}


GPU2 = [{"DiscreteResourceSpec": {"Kind": "gpu", "Value": 2}}]
GPU_TWICE = [{"DiscreteResourceSpec": {"Kind": "gpu", "Value": 2}}, {"DiscreteResourceSpec": {"Kind": "gpu", "Value": 1}}]
WANT_GPU = {"Resources": {"Reservations": {"NanoCPUs": 10**9, "Generic": [{"DiscreteResourceSpec": {"Kind": "gpu", "Value": 1}}]}}}


@pytest.mark.parametrize("seed", range(12))
def test_batched_preassigned_path_decides_as_the_per_task_path(seed):
    rng = random.Random(0xF17 + seed)
    p = FitPair()
    n_nodes = rng.choice([1, 4, 17, 40])
    nodes = {}
    for i in range(n_nodes):
        r = rng.random()
        d = _node(i, GPU2 if r < 0.2 else GPU_TWICE if r < 0.3 else None)
        if rng.random() < 0.15:
            d["Spec"]["Availability"] = rng.choice([1, 2])
        nodes[i] = d
        p.both("create_node", d)
    sids = ["svc%02d" % k for k in range(rng.randrange(1, 6))] + (["boom-pre"] if rng.random() < 0.4 else [])
    for sid in sids:
        p.both("set_service", sid)
    specs = {sid: rng.choice([None, WANT_GPU, _mounts(), {"Placement": {"MaxReplicas": rng.choice([1, 2])}},
                              {"Placement": {"Preferences": [{"Spread": {"SpreadDescriptor": "node.labels.zone"}}]}}, None]) for sid in sids}
    tid = 0
    placed = {}
    for rnd in range(rng.randrange(2, 5)):
        for _ in range(rng.randrange(1, 4)):   # global-service style: one task per node of a service, some extra on a node
            sid = rng.choice(sids)
            for i in sorted(nodes):
                for _ in range(rng.choice([1, 1, 1, 2, 3])):
                    kw = {}
                    if specs[sid] is not None:
                        kw["Spec"] = dict(specs[sid])
                    if rng.random() < 0.1:
                        kw["Endpoint"] = {"Ports": [{"Protocol": 0, "PublishedPort": rng.choice([80, 8080]), "PublishMode": 1}]}
                    if rng.random() < 0.1:
                        kw["DesiredState"] = orc.SHUTDOWN
                    t = _task("t%05d" % tid, sid, nodes[i]["ID"] if rng.random() > 0.05 else "n-unknown", **kw)
                    tid += 1
                    p.both("create_task", t)
                    if rng.random() < 0.03:   # the same id again, already on its node: addTask's state-change branches
                        p.both("create_task", dict(t, Status={"State": orc.RUNNING}))
                        p.both("create_task", t)
        for d in p.both("process_preassigned"):
            if d["NodeID"] and d["State"] >= orc.ASSIGNED and not d.get("Deferred"):
                placed[d["ID"]] = d["NodeID"]
        if placed and rng.random() < 0.5:   # resources freed on a node: the pending tasks are checked again
            for t in rng.sample(sorted(placed), min(len(placed), rng.randrange(1, 6))):
                p.both("delete_task", {"ID": t, "ServiceID": "x", "NodeID": placed.pop(t), "Status": {"State": orc.RUNNING}})
        if rng.random() < 0.3:
            i = rng.choice(sorted(nodes))
            nodes[i] = dict(nodes[i], Spec={"Availability": rng.choice([0, 0, 1])})
            p.both("update_node", nodes[i])
        p.both("process_preassigned")
        p.both("tick")
    for i in sorted(nodes)[:8]:
        p.both("node_info", nodes[i]["ID"])


def test_one_fit_call_per_run_of_tasks():
    p = FitPair()
    for i in range(3):
        p.both("create_node", _node(i))
    p.both("create_node", _node(3, GPU_TWICE))
    for sid in ("a", "b", "vol"):
        p.both("set_service", sid)
    for i in range(3):
        p.both("create_task", _task("a%d" % i, "a", "n%03d" % i))
    c0 = p.calls()
    d = p.both("process_preassigned")
    assert [x["ID"] for x in d] == ["a0", "a1", "a2"]
    assert p.calls() == c0 + 1                    # one run, one call
    # a mount task between two runs: the run before it is flushed first
    p.both("create_task", _task("b0", "b", "n000"))
    p.both("create_task", _task("v0", "vol", "n001", Spec=_mounts()))
    p.both("create_task", _task("b1", "b", "n001"))
    c0 = p.calls()
    p.both("process_preassigned")
    assert p.calls() == c0 + 2                    # b0, then v0 on its own, then b1
    # only tasks the batched call does not stand for: no call at all
    p2 = FitPair()
    for i in range(2):
        p2.both("create_node", _node(i))
    p2.both("create_node", _node(2, GPU_TWICE))
    p2.both("set_service", "vol")
    p2.both("set_service", "g")
    p2.both("set_service", "r")
    p2.both("create_task", _task("v1", "vol", "n000", Spec=_mounts()))
    p2.both("create_task", _task("g1", "g", "n002", Spec=WANT_GPU))            # an irregular generic kind on its node
    t = _task("r1", "r", "n001")
    p2.both("create_task", dict(t, Status={"State": orc.RUNNING}))
    p2.both("create_task", t)                                                  # already in its node's Tasks
    c0 = p2.calls()
    d = p2.both("process_preassigned")
    assert {x["ID"] for x in d} == {"v1", "g1", "r1"}
    assert p2.calls() == c0


def test_a_refused_fit_call_takes_the_per_task_path():
    p = FitPair()
    p.both("create_node", _node(0))
    for sid in ("ok", "boom-pre"):
        p.both("set_service", sid)
    for tid, sid in (("p1", "ok"), ("pb", "boom-pre"), ("p2", "ok")):
        p.both("create_task", _task(tid, sid, "n000"))
    c0 = p.calls()
    d = p.both("process_preassigned")
    by = {x["ID"]: x for x in d}
    assert by["pb"].get("Deferred") is True and "refused" in by["pb"]["Err"]
    assert not by["p1"].get("Deferred") and not by["p2"].get("Deferred")
    assert p.calls() == c0 + 1
