"""GPU: swp_fit_pairs (k_fit_pairs) — taskFitNode for many preassigned tasks in one device pass — against what it stands for: a loop
of swp_check_node + swp_commit (+ swp_node_set_generic with the count less the request) per passing pair on a twin engine fed the same
events. Engine level: first_fail per pair, then every node's row, per-service counts and generic counts. Host level: the product's
processPreassignedTasks (now batched through swp_fit_pairs) against the CPU oracle, on one engine and over shard sets."""
import random

import numpy as np
import pytest

import bigcases
import orc
import test_engine_fuzz as fz
from swarmkit_amd import abi, sched as swsched
from swarmkit_amd import host as swhost

pytestmark = pytest.mark.gpu

KINDS = ("gpu", "fpga")


def _node(rng, i):
    d = fz.node_doc(rng, i)
    if rng.random() < 0.3:
        d["Description"]["Resources"]["Generic"] = [{"DiscreteResourceSpec": {"Kind": k, "Value": rng.randrange(1, 6)}} for k in KINDS if rng.random() < 0.7]
    return d


def _template(rng, k):
    t = fz.service_spec(rng)
    spec = t.setdefault("Spec", {})
    (spec.get("Placement") or {}).pop("Preferences", None)   # (spread preferences: swp_check_node and swp_fit_pairs refuse them alike)
    res = spec.setdefault("Resources", {}).setdefault("Reservations", {})
    r = rng.random()
    if r < 0.3:
        res["Generic"] = [{"DiscreteResourceSpec": {"Kind": kd, "Value": rng.randrange(1, 3)}} for kd in KINDS if rng.random() < 0.6] or \
                         [{"DiscreteResourceSpec": {"Kind": "gpu", "Value": 1}}]
    if rng.random() < 0.25:
        t["Endpoint"] = {"Ports": [{"Protocol": rng.choice([0, 1]), "PublishedPort": 9000 + rng.randrange(3), "PublishMode": 1} for _ in range(rng.randrange(1, 3))]}
    if rng.random() < 0.25:
        spec.setdefault("Placement", {})["MaxReplicas"] = rng.choice([1, 2, 3, 5])
    if rng.random() < 0.15:
        spec["LogDriver"] = {"Name": "syslog"}   # PluginFilter: a log driver the node must have
    t.update({"ID": "tmpl%d" % k, "ServiceID": "svc%02d" % (k % 7), "Status": {"State": orc.PENDING},
              "DesiredState": orc.SHUTDOWN if rng.random() < 0.15 else orc.RUNNING})   # SHUTDOWN: SWP_TASK_UNCOUNTED
    return t


def _cluster(rng, N, shards=None):
    """Two schedulers over real engines (or shard sets) with the same nodes; returns them, the node docs and the template docs."""
    kw = {} if not shards else {"shards": shards, "nodes_per_shard": (N + shards - 1) // shards + 2}
    a, b = swsched.Scheduler(**kw), swsched.Scheduler(**kw)
    docs = [_node(rng, i) for i in range(N)]
    for d in docs:
        a.create_node(d)
        b.create_node(d)
    for k in range(7):
        a.set_service("svc%02d" % k)
        b.set_service("svc%02d" % k)
    return a, b, docs


def _descs(s, tdocs):
    return np.concatenate([s.task_desc(t) for t in tdocs])


def _loop(e, tmpls, pairs, kinds):
    """What swp_fit_pairs stands for, one pair at a time."""
    ff = np.empty(len(pairs), dtype=np.int32)
    for i, (node, ti) in enumerate(pairs):
        t = tmpls[ti]
        ff[i] = e.check_node(t, node)
        if ff[i] != -1:
            continue
        e.commit(np.array([(node, t["service"], t["cpu"], t["mem"], t["port_set"], 0 if t["flags"] & abi.TASK_UNCOUNTED else 1)], dtype=abi.PLACEMENT_DTYPE))
        if t["generic_set"]:
            want = dict(_gen_items(e, t))
            counts = []
            for kid in kinds:
                c = e.node_get_generic(node, kid)
                c = max(c - want.get(kid, 0), 0)
                if c > 0:
                    counts.append((kid, c))
            e.node_set_generic(node, counts)
    return ff


_GEN = {}


def _gen_items(e, t):
    return _GEN[(id(e), int(t["generic_set"]))]


def _state(e, nodes, services, kinds):
    rows = e.node_get_many(nodes)
    svc = [[e.node_get_svc_count(n, s) for s in services] for n in nodes]
    gen = [[e.node_get_generic(n, k) for k in kinds] for n in nodes]
    return rows[["cpu", "mem", "total", "flags"]].tolist(), svc, gen


def _gen_table(s, e, tdocs, descs):
    for t, d in zip(tdocs, descs):
        gs = int(d["generic_set"])
        if gs:
            g = (((t.get("Spec") or {}).get("Resources") or {}).get("Reservations") or {}).get("Generic") or []
            _GEN[(id(e), gs)] = [(e.intern(abi.SPACE_GENERIC_KIND, x["DiscreteResourceSpec"]["Kind"]), x["DiscreteResourceSpec"]["Value"]) for x in g]


@pytest.mark.parametrize("seed,N,shards", [(0, 1000, None), (1, 3000, None), (2, 10000, None), (3, 2000, 3), (4, 1000, None), (5, 4000, 2)])
def test_fit_pairs_equals_the_check_commit_loop(seed, N, shards):
    rng = random.Random(0xF1700 + seed)
    a, b, docs = _cluster(rng, N, shards)
    tdocs = [_template(rng, k) for k in range(rng.randrange(3, 12))]
    da, db = _descs(a, tdocs), _descs(b, tdocs)
    assert da.tobytes() == db.tobytes()
    _gen_table(a, a.e, tdocs, da)
    _gen_table(b, b.e, tdocs, db)
    idx = [a.node_index(d["ID"]) for d in docs]
    assert idx == [b.node_index(d["ID"]) for d in docs]
    hot = rng.sample(idx, 4)   # segments longer than 64 pairs: cpu / mem / generic counts / ports / MaxReplicas run out on the way
    pairs = []
    for _ in range(rng.randrange(N // 2, 2 * N)):
        pairs.append((rng.choice(hot) if rng.random() < 0.1 else rng.choice(idx), rng.randrange(len(tdocs))))
    rng.shuffle(pairs)
    kinds = [a.e.intern(abi.SPACE_GENERIC_KIND, k) for k in KINDS]
    services = sorted({int(d["service"]) for d in da})
    got = a.e.fit_pairs(da, pairs)
    want = _loop(b.e, db, pairs, kinds)
    assert (got == want).all(), [(i, pairs[i], got[i], want[i]) for i in np.nonzero(got != want)[0][:5]]
    assert (got == -1).any() and (got >= 0).any()
    assert _state(a.e, idx, services, kinds) == _state(b.e, idx, services, kinds)
    # the state afterwards is what later calls read: a second round on the changed nodes agrees too
    pairs2 = [(rng.choice(hot), rng.randrange(len(tdocs))) for _ in range(200)]
    assert (a.e.fit_pairs(da, pairs2) == _loop(b.e, db, pairs2, kinds)).all()
    assert _state(a.e, idx, services, kinds) == _state(b.e, idx, services, kinds)


@pytest.mark.parametrize("shards", [None, 2])
def test_state_restore_undoes_a_fit_call_and_a_refused_call_applies_nothing(shards):
    rng = random.Random(77)
    a, _, docs = _cluster(rng, 1500, shards)
    tdocs = [_template(rng, k) for k in range(6)]
    da = _descs(a, tdocs)
    idx = [a.node_index(d["ID"]) for d in docs]
    kinds = [a.e.intern(abi.SPACE_GENERIC_KIND, k) for k in KINDS]
    services = sorted({int(d["service"]) for d in da})
    pairs = [(rng.choice(idx[:50]), rng.randrange(len(tdocs))) for _ in range(3000)]
    before = _state(a.e, idx, services, kinds)
    a.e.state_save()
    ff = a.e.fit_pairs(da, pairs)
    assert (ff == -1).any()
    assert _state(a.e, idx, services, kinds) != before
    a.e.state_restore()
    assert _state(a.e, idx, services, kinds) == before
    # refused: a template with cluster mounts, a node that is not there, a template index out of range — nothing applied
    bad = da.copy()
    bad[0]["flags"] |= 1 << 8
    with pytest.raises(abi.SwpError) as err:
        a.e.fit_pairs(bad, pairs)
    assert err.value.code == abi.SWP_EUNSUPPORTED
    with pytest.raises(abi.SwpError):
        a.e.fit_pairs(da, pairs + [(max(idx) + 10, 0)])
    with pytest.raises(abi.SwpError):
        a.e.fit_pairs(da, pairs + [(idx[0], len(tdocs))])
    assert _state(a.e, idx, services, kinds) == before
    assert (a.e.fit_pairs(da, pairs) == ff).all()   # (the same call on the same state: the same verdicts)


# ------------------------------------------------------------------------------------------------ host level, against the oracle
def _host_script(x, rng_seed, N, services, per_node):
    """Global services (one preassigned task per node each, some nodes more), then node updates that free resources and a second
    pass; mount and deferred tasks mixed into the pending list. Returns what the caller compares."""
    rng = random.Random(rng_seed)
    out = []
    docs = [fz.node_doc(rng, i) for i in range(N)]
    for d in docs:
        x.create_node(d)
    x.update_volume({"ID": "v0", "Spec": {"Annotations": {"Name": "vol0"}, "Group": "g", "Driver": {"Name": "csi-a"},
                                          "AccessMode": {"Scope": "MULTI_NODE", "Sharing": "ALL"}, "Availability": "ACTIVE"},
                     "VolumeInfo": {"VolumeID": "plug0", "AccessibleTopology": []}})
    specs = []
    for k in range(services):
        sp = fz.service_spec(rng)
        (sp.get("Spec", {}).get("Placement") or {}).pop("Preferences", None)
        if k % 4 == 3:   # cluster mounts: the per-task path inside the batched walk
            sp.setdefault("Spec", {})["Container"] = {"Mounts": [{"Type": "CLUSTER", "Source": "group:g", "Target": "/d"}]}
        specs.append(sp)
        x.set_service("gs%02d" % k)
    tid = 0
    for k in range(services):
        for i in range(N):
            for _ in range(per_node if i % 5 == 0 else 1):
                t = dict(specs[k], ID="g%02d-%06d" % (k, tid), ServiceID="gs%02d" % k, NodeID=docs[i]["ID"], DesiredState=orc.RUNNING,
                         Status={"State": orc.PENDING})
                if rng.random() < 0.05:
                    t["DesiredState"] = orc.SHUTDOWN
                x.create_task(t)
                tid += 1
    key = lambda d: d["ID"]
    line = lambda d: (d["ID"], d["NodeID"], d["State"], d["Err"], d.get("AssignedGenericResources"), bool(d.get("Deferred")))
    out.append(sorted(map(line, x.process_preassigned()), key=lambda r: r[0]))
    for i in range(0, N, 3):   # more room on a third of the nodes: the pending tasks are checked again
        d = dict(docs[i])
        d["Description"] = dict(d["Description"], Resources={"NanoCPUs": 64 * 10**9, "MemoryBytes": 256 << 30})
        x.create_node(d)
    out.append(sorted(map(line, x.process_preassigned()), key=lambda r: r[0]))
    for j in range(300):   # one-off tasks: the tick after sees the nodes as the preassigned tasks left them
        x.create_task(dict(specs[j % services], ID="o%05d" % j, ServiceID="gs%02d" % (j % services), DesiredState=orc.RUNNING, Status={"State": orc.PENDING}))
    out.append(bigcases.tick_digest(x.tick()))
    for i in range(0, N, max(1, N // 25)):
        info = x.node_info(docs[i]["ID"])
        out.append((info["ActiveTasksCount"], info["AvailableResources"]["NanoCPUs"], info["AvailableResources"]["MemoryBytes"],
                    sorted(info["ActiveTasksCountByService"].items())))
    return out


@pytest.mark.parametrize("shards", [None, 2, 3, 4])
@pytest.mark.parametrize("seed", [0, 1])
def test_process_preassigned_matches_the_oracle(seed, shards):
    N = 400
    kw = {} if not shards else {"shards": shards, "nodes_per_shard": N // shards + 3}
    want = _host_script(orc.Oracle(), 0xA55 + seed, N, 6, 3)
    got = _host_script(swhost.HostScheduler(**kw), 0xA55 + seed, N, 6, 3)
    assert got == want


def test_ten_thousand_nodes_five_global_services():
    want = _host_script(orc.Oracle(), 0xB16, 10000, 5, 1)
    got = _host_script(swhost.HostScheduler(), 0xB16, 10000, 5, 1)
    assert got == want
