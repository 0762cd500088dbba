"""GPU: swp_fit_pairs_volumes (k_fit_pairs_vol) — taskFitNode for many preassigned tasks, cluster mounts included, in one device pass —
against the CPU oracle. Engine level: a seeded cluster with CSI infos and topologies, volumes of every scope x sharing x availability
(some in use from start-up, a single-node one among them), templates with 1-8 mounts incl. `group:` sources next to templates without;
the expected first_fail / attachment rows are the oracle's processPreassignedTasks over the same tasks in pair order (its taskFitNode:
oracle/swk_oracle.cpp), cross-checked with swp_check_node + swp_choose_volumes + swp_commit per pair on a second engine. Host level: the
C++ host layer's processPreassignedTasks (mount tasks inside the run) against the oracle. On one engine and over shard sets.

Seeds: every seed of both tests reaches mount pairs in the ORACLE's script (a seed would be skipped only if it did not); with the
generator below — 3 of 4 templates mount something — the oracle alone, checked on the CPU over the seeds used here, reaches a mount pair
that passes filters 0..6 in 100 % of them (share skipped: 0 %, the cap is 10 %)."""
import ctypes as C
import random

import numpy as np
import pytest

import bigcases
import orc
import test_engine_fuzz as fz
from swarmkit_amd import abi, sched as swsched
from swarmkit_amd import host as swhost

pytestmark = pytest.mark.gpu

ZONES = ["z1", "z2", "z3"]
SCOPES = ["SINGLE_NODE", "MULTI_NODE"]
SHARINGS = ["NONE", "READ_ONLY", "ONE_WRITER", "ALL"]
GROUPS = ["ga", "gb", "gc"]
N_VOL = 2 * 4 * 2 + 4   # every scope x sharing x availability once, then a few more


@pytest.fixture(autouse=True)
def cxx_host(monkeypatch):
    monkeypatch.setenv("SWP_HOST", "cxx")   # (the Python twin of the host layer keeps its per-task path)


def _node(rng, i):
    d = fz.node_doc(rng, i)
    csi = []
    for plug in ("p1", "p2"):
        if rng.random() < 0.85:
            c = {"PluginName": plug, "NodeID": "csi-%s-%d" % (plug, i)}
            if rng.random() < 0.8:
                c["AccessibleTopology"] = {"Segments": {"zone": rng.choice(ZONES), **({"rack": rng.choice("ab")} if rng.random() < 0.4 else {})}}
            csi.append(c)
    d["Description"]["CSIInfo"] = csi
    return d


def _volumes(rng):
    out = []
    for v in range(N_VOL):
        scope, sharing, avail = SCOPES[v % 2], SHARINGS[(v // 2) % 4], "PAUSE" if (v // 8) % 2 and v < 16 else "ACTIVE"
        acc = [{"Segments": {"zone": rng.choice(ZONES), **({"rack": rng.choice("ab")} if rng.random() < 0.3 else {})}} for _ in range(rng.choice([0, 1, 1, 2]))]
        out.append({"ID": "vol%02d" % v, "Spec": {"Annotations": {"Name": "name%02d" % v}, "Group": rng.choice(GROUPS), "Driver": {"Name": rng.choice(["p1", "p2"])},
                                                  "AccessMode": {"Scope": scope, "Sharing": sharing}, "Availability": avail},
                    "VolumeInfo": {"VolumeID": "csi%02d" % v, "AccessibleTopology": acc}})
    # vol20: a single-node volume every node's topology fits — its users (below) pin it to one node
    out.append({"ID": "vol%02d" % N_VOL, "Spec": {"Annotations": {"Name": "pinned"}, "Group": "gpin", "Driver": {"Name": "p1"},
                                                  "AccessMode": {"Scope": "SINGLE_NODE", "Sharing": "ALL"}, "Availability": "ACTIVE"},
                "VolumeInfo": {"VolumeID": "csi-pinned", "AccessibleTopology": []}})
    return out


def _mounts(rng, k):
    """1-8 cluster mounts: named and `group:` sources, read-only ones, names and groups that do not exist, sometimes a bind mount between."""
    if k == 0:
        return [{"Type": "CLUSTER", "Source": "pinned", "Target": "/pin"}]
    if k == 1:
        return [{"Type": "CLUSTER", "Source": "group:gpin", "Target": "/pin", "ReadOnly": True}, {"Type": "CLUSTER", "Source": "group:ga", "Target": "/a"}]
    ms = []
    for m in range(rng.choice([1, 1, 2, 2, 3, 5, 8])):
        src = rng.choice(["name%02d" % rng.randrange(N_VOL + 1), "group:" + rng.choice(GROUPS + GROUPS + ["gnone"])])
        ms.append({"Type": "CLUSTER", "Source": src, "Target": "/m%d" % rng.randrange(4), "ReadOnly": rng.random() < 0.4})
    if rng.random() < 0.2:
        ms.insert(rng.randrange(len(ms) + 1), {"Type": "BIND", "Source": "/x", "Target": "/y"})
    return ms


def _template(rng, k):
    t = fz.service_spec(rng)
    spec = t.setdefault("Spec", {})
    (spec.get("Placement") or {}).pop("Preferences", None)
    if rng.random() < 0.5:                      # most nodes should reach the volumes: few constraints
        spec.pop("Placement", None)
    if rng.random() < 0.2:
        t["Endpoint"] = {"Ports": [{"Protocol": 0, "PublishedPort": 9000 + rng.randrange(3), "PublishMode": 1}]}
    if rng.random() < 0.2:
        spec.setdefault("Placement", {})["MaxReplicas"] = rng.choice([1, 2, 3])
    if k % 4 != 3:
        spec["Container"] = {"Mounts": _mounts(rng, k)}
    t.update({"ServiceID": "svc%02d" % (k % 7), "Status": {"State": orc.PENDING}, "DesiredState": orc.SHUTDOWN if rng.random() < 0.1 else orc.RUNNING})
    return t


def _script(rng, N):
    """Node docs, volume docs, running tasks that hold volumes from start-up, template docs."""
    nodes = [_node(rng, i) for i in range(N)]
    vols = _volumes(rng)
    users = []
    pin = nodes[N - 2]["ID"]                    # (a node of the LAST shard of every shard set used here)
    users.append({"ID": "u-pin", "ServiceID": "users", "NodeID": pin, "DesiredState": orc.RUNNING, "Status": {"State": orc.RUNNING},
                  "Spec": {"Container": {"Mounts": [{"Type": "CLUSTER", "Source": "pinned", "Target": "/pin"}]}},
                  "Volumes": [{"ID": "vol%02d" % N_VOL, "Source": "pinned", "Target": "/pin"}]})
    for u in range(12):                         # users of other volumes, writers and readers, on any node (the checks only read them)
        v = rng.randrange(N_VOL)
        ro = rng.random() < 0.5
        users.append({"ID": "u%02d" % u, "ServiceID": "users", "NodeID": rng.choice(nodes)["ID"], "DesiredState": orc.RUNNING, "Status": {"State": orc.RUNNING},
                      "Spec": {"Container": {"Mounts": [{"Type": "CLUSTER", "Source": "name%02d" % v, "Target": "/u", "ReadOnly": ro}]}},
                      "Volumes": [{"ID": "vol%02d" % v, "Source": "name%02d" % v, "Target": "/u"}]})
    tdocs = [_template(rng, k) for k in range(rng.randrange(6, 13))]
    return nodes, vols, users, tdocs


def _load(x, nodes, vols, users):
    for d in nodes:
        x.create_node(d)
    for v in vols:
        x.update_volume(v)
    for k in range(7):
        x.set_service("svc%02d" % k)
    x.set_service("users")
    for u in users:
        x.setup_task(u)


def _choose(e, mset, node):
    out, n, failed = (C.c_uint32 * abi.MAX_MOUNTS)(), C.c_uint32(), C.c_uint32()
    e.L.swp_choose_volumes.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    e._ck(e.L.swp_choose_volumes(e.h, mset, node, out, C.byref(n), C.byref(failed)))
    return list(out), n.value


def _loop(e, tmpls, pairs):
    """What the call stands for, one pair at a time: swp_check_node, swp_choose_volumes, swp_commit."""
    ff = np.empty(len(pairs), dtype=np.int32)
    att = np.full((len(pairs), abi.MAX_MOUNTS), abi.NO_VOLUME, dtype=np.uint32)
    for i, (node, ti) in enumerate(pairs):
        t = tmpls[ti]
        ff[i] = e.check_node(t, node)
        if ff[i] != -1:
            continue
        mset = int(t["flags"]) >> 8
        if mset:
            row, n = _choose(e, mset, node)
            att[i] = row
            if n == 0:
                ff[i] = abi.FIT_NO_VOLUME
                continue
        e.commit(np.array([(node, t["service"], t["cpu"], t["mem"], t["port_set"], 0 if t["flags"] & abi.TASK_UNCOUNTED else 1)], dtype=abi.PLACEMENT_DTYPE))
    return ff, att


def _oracle_rows(o, s, tdocs, pairs, ids, vol_index):
    """The oracle's taskFitNode over the pairs in pair order (pending tasks are walked in ascending ID) as first_fail / attachment rows."""
    for i, (node, ti) in enumerate(pairs):
        o.create_task(dict(tdocs[ti], ID="p%07d" % i, NodeID=ids[node]))
    filt = {s.explain([1 if k == f else 0 for k in range(8)]): f for f in range(8)}
    ff = np.full(len(pairs), -99, dtype=np.int32)
    att = np.full((len(pairs), abi.MAX_MOUNTS), abi.NO_VOLUME, dtype=np.uint32)
    for d in o.process_preassigned():
        i = int(d["ID"][1:])
        if d["State"] == orc.ASSIGNED:
            ff[i] = -1
            for m, v in enumerate(d.get("Volumes") or []):
                att[i, m] = vol_index[v["ID"]]
        elif d["Err"].startswith("cannot find volume to satisfy mount"):
            ff[i] = abi.FIT_NO_VOLUME
            for m, v in enumerate(d.get("VolumePrefix") or []):
                att[i, m] = vol_index[v]
        else:
            ff[i] = filt[d["Err"]]
    return ff, att


def _usage(e, vol_index):
    return [e.volume_get_usage(v) for v in sorted(vol_index.values())]


def _state(e, idx, services):
    rows = e.node_get_many(idx)
    return rows[["cpu", "mem", "total", "flags"]].tolist(), [[e.node_get_svc_count(n, sv) for sv in services] for n in idx]


@pytest.mark.parametrize("seed,N,shards", [(0, 600, None), (1, 1500, None), (2, 900, 2), (3, 900, 3), (4, 1200, 4), (5, 3000, None)])
def test_fit_pairs_volumes_equals_the_oracle_and_the_per_pair_loop(seed, N, shards):
    rng = random.Random(0x701F00 + seed)
    kw = {} if not shards else {"shards": shards, "nodes_per_shard": (N + shards - 1) // shards + 2}
    a, b, o = swsched.Scheduler(**kw), swsched.Scheduler(**kw), orc.Oracle()
    nodes, vols, users, tdocs = _script(rng, N)
    for x in (a, b, o):
        _load(x, nodes, vols, users)
    da = np.concatenate([a.task_desc(t) for t in tdocs])
    db = np.concatenate([b.task_desc(t) for t in tdocs])
    assert da.tobytes() == db.tobytes() and (da["flags"] >> 8).any()
    ids = {a.node_index(d["ID"]): d["ID"] for d in nodes}
    idx = sorted(ids)
    vol_index = {v["ID"]: a.e.intern(abi.SPACE_VOLUME, v["ID"]) for v in vols}
    if shards:   # the pinned single-node volume is in use on a node of the last shard: the other shards hold a foreign pin
        per = kw["nodes_per_shard"]
        assert a.node_index(nodes[N - 2]["ID"]) // per == shards - 1 and a.e.volume_get_usage(vol_index["vol%02d" % N_VOL])[0] == 1
    hot = rng.sample(idx, 4)
    pairs = [(rng.choice(hot) if rng.random() < 0.05 else rng.choice(idx), rng.randrange(len(tdocs))) for _ in range(rng.randrange(N, 3 * N))]
    pairs += [(i, 0) for i in idx[:: max(1, N // 64)]] + [(a.node_index(nodes[N - 2]["ID"]), 0), (a.node_index(nodes[N - 2]["ID"]), 1)]   # the pinned volume from every shard
    services = sorted({int(d["service"]) for d in da})
    use0, before = _usage(a.e, vol_index), _state(a.e, idx, services)
    want_ff, want_att = _oracle_rows(o, a, tdocs, pairs, ids, vol_index)
    reached = [i for i, (n, t) in enumerate(pairs) if da[t]["flags"] >> 8 and (want_ff[i] == -1 or want_ff[i] >= 7)]
    if not reached:
        pytest.skip("the oracle's script reaches no mount pair")
    a.e.state_save()
    ff, att = a.e.fit_pairs_volumes(da, pairs)
    bad = np.nonzero(ff != want_ff)[0]
    assert not len(bad), [(int(i), pairs[i], int(ff[i]), int(want_ff[i])) for i in bad[:6]]
    bad = np.nonzero((att != want_att).any(axis=1))[0]
    assert not len(bad), [(int(i), pairs[i], int(ff[i]), att[i].tolist(), want_att[i].tolist()) for i in bad[:6]]
    assert (ff == -1).any() and (ff == 7).any() and ((ff >= 0) & (ff < 7)).any()
    loop_ff, loop_att = _loop(b.e, db, pairs)
    assert (loop_ff == ff).all() and (loop_att == att).all()
    assert _usage(a.e, vol_index) == use0 == _usage(b.e, vol_index)          # taskFitNode reserves nothing
    after = _state(a.e, idx, services)
    assert after == _state(b.e, idx, services) and after != before
    # a pinned volume: only pairs on its node may get it (from another shard: a foreign pin equals no local node)
    pinned, pin_node = vol_index["vol%02d" % N_VOL], a.node_index(nodes[N - 2]["ID"])
    assert all(pairs[i][0] == pin_node for i in np.nonzero((att == pinned).any(axis=1))[0])
    # state_restore undoes the call; a refused call applies nothing
    a.e.state_restore()
    assert _state(a.e, idx, services) == before
    spread = da.copy()
    spread[0]["spread_set"] = 1
    for templates, prs in ((da, pairs + [(max(idx) + 10, 0)]), (da, pairs + [(idx[0], len(tdocs))]), (spread, pairs)):
        with pytest.raises(abi.SwpError):
            a.e.fit_pairs_volumes(templates, prs)
    unknown = da.copy()
    unknown[0]["flags"] |= 0xFFFFF << 8
    with pytest.raises(abi.SwpError):
        a.e.fit_pairs_volumes(unknown, pairs)
    assert _state(a.e, idx, services) == before and _usage(a.e, vol_index) == use0
    ff2, att2 = a.e.fit_pairs_volumes(da, pairs)
    assert (ff2 == ff).all() and (att2 == att).all()


@pytest.mark.parametrize("shards", [None, 3])
def test_a_call_without_mount_templates_returns_what_fit_pairs_returns(shards):
    rng = random.Random(0x70177)
    N = 800
    kw = {} if not shards else {"shards": shards, "nodes_per_shard": N // shards + 3}
    a, b = swsched.Scheduler(**kw), swsched.Scheduler(**kw)
    nodes, vols, users, tdocs = _script(rng, N)
    for x in (a, b):
        _load(x, nodes, vols, users)
    plain = [t for t in tdocs if "Container" not in t.get("Spec", {})] + [dict(fz.service_spec(rng), ServiceID="svc00", DesiredState=orc.RUNNING, Status={"State": orc.PENDING})]
    for t in plain:
        (t.get("Spec", {}).get("Placement") or {}).pop("Preferences", None)
    da, db = np.concatenate([a.task_desc(t) for t in plain]), np.concatenate([b.task_desc(t) for t in plain])
    idx = [a.node_index(d["ID"]) for d in nodes]
    pairs = [(rng.choice(idx), rng.randrange(len(plain))) for _ in range(2000)]
    ff, att = a.e.fit_pairs_volumes(da, pairs)
    assert (ff == b.e.fit_pairs(db, pairs)).all() and (att == abi.NO_VOLUME).all()
    services = sorted({int(d["service"]) for d in da})
    assert _state(a.e, idx, services) == _state(b.e, idx, services)


# ------------------------------------------------------------------------------------------------ host level, against the oracle
def _host_script(x, rng_seed, N, services, per_node):
    """tests/test_engine_preassigned.py's script with mounts on most services and the volumes above: global services (one preassigned
    task per node each, some nodes more), node updates that free resources and a second pass, the tick after; then the books."""
    rng = random.Random(rng_seed)
    out = []
    nodes, vols, users, _ = _script(rng, N)
    _load(x, nodes, vols, users)
    specs = []
    for k in range(services):
        sp = _template(rng, k if k % 4 != 3 else k)
        specs.append(sp)
        x.set_service("gs%02d" % k)
    tid = 0
    for k in range(services):
        for i in range(N):
            for _ in range(per_node if i % 5 == 0 else 1):
                t = dict(specs[k], ID="g%02d-%06d" % (k, tid), ServiceID="gs%02d" % k, NodeID=nodes[i]["ID"], DesiredState=orc.RUNNING, Status={"State": orc.PENDING})
                if rng.random() < 0.05:
                    t["DesiredState"] = orc.SHUTDOWN
                x.create_task(t)
                tid += 1
    line = lambda d: (d["ID"], d["NodeID"], d["State"], d["Err"], d.get("AssignedGenericResources"), bool(d.get("Deferred")),
                      tuple((v["ID"], v["Source"], v["Target"]) for v in d.get("Volumes") or ()))
    out.append(sorted(map(line, x.process_preassigned())))
    for i in range(0, N, 3):   # more room on a third of the nodes: the pending tasks are checked again
        d = dict(nodes[i])
        d["Description"] = dict(d["Description"], Resources={"NanoCPUs": 64 * 10**9, "MemoryBytes": 256 << 30})
        x.create_node(d)
    out.append(sorted(map(line, x.process_preassigned())))
    for j in range(200):
        x.create_task(dict(specs[j % services], ID="o%05d" % j, ServiceID="gs%02d" % (j % services), DesiredState=orc.RUNNING, Status={"State": orc.PENDING}))
    out.append(bigcases.tick_digest(x.tick()))
    for i in range(0, N, max(1, N // 25)):
        info = x.node_info(nodes[i]["ID"])
        out.append((info["ActiveTasksCount"], info["AvailableResources"]["NanoCPUs"], info["AvailableResources"]["MemoryBytes"],
                    sorted(info["ActiveTasksCountByService"].items())))
    for v in vols:
        info = x.volume_info(v["ID"])
        out.append((v["ID"], info["Tasks"], {k: c for k, c in info["Nodes"].items() if c}))
    out.append(x.free_volumes())
    return out


@pytest.mark.parametrize("shards", [None, 2, 3, 4])
@pytest.mark.parametrize("seed", [0, 1])
def test_process_preassigned_with_mounts_matches_the_oracle(seed, shards):
    N = 400
    kw = {} if not shards else {"shards": shards, "nodes_per_shard": N // shards + 3}
    want = _host_script(orc.Oracle(), 0xA77 + seed, N, 8, 3)
    mounted = [r for r in want[0] + want[1] if r[6] or r[3].startswith("cannot find volume")]
    if not mounted:
        pytest.skip("the oracle's script reaches no mount pair")
    got = _host_script(swhost.HostScheduler(**kw), 0xA77 + seed, N, 8, 3)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, [(x, y) for x, y in zip(g, w) if x != y][:3] if isinstance(g, list) else (g, w))
