"""GPU: the streamed run (include/swp.h swp_batch_run_streamed / swp_schedule_batch_streamed) — k_publish copies the decided prefix of
a running batch to host-visible memory behind every SWP_STREAM_EVERY rounds, every scan stretch and every k_waterfill run, and the
caller's sink receives it, folded into the node mirror, while later rounds run.

Through the struct ABI, judged by the oracle (tests/orc.py) as test_engine_parity.py does. For every case: the ranges the sink saw are
contiguous, ascending, cover the batch once and respect min_tasks; put together they are what a plain swp_schedule_batch gives on a twin
engine, and what the oracle decides; the Explain rows and the attachments are the plain run's; every node row reads the same afterwards.
The oracle's answer for a cluster is computed once and shared."""
import json
import os
import random
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
GIB = 1 << 30


@pytest.fixture(autouse=True)
def cxx_host(monkeypatch):
    monkeypatch.setenv("SWP_HOST", "cxx")   # (the Python twin of the host layer knows no volumes)
    for k in ("SWP_R6_BLOCK", "SWP_STREAM_EVERY", "SWP_SCAN", "SWP_WATERFILL"):
        monkeypatch.delenv(k, raising=False)


class Cluster:
    """Node, volume and task documents in order: the same into the oracle and into an engine."""

    def __init__(self, key, nodes, services, tasks, volumes=()):
        self.key, self.nodes, self.services, self.tasks, self.volumes = key, list(nodes), list(services), list(tasks), list(volumes)

    @classmethod
    def of_workload(cls, key, wl, extra_tasks=()):
        return cls(key, wl.node_docs(), [wl.service_id(k) for k in range(wl.S)], wl.task_docs() + list(extra_tasks))

    @property
    def T(self):
        return len(self.tasks)


_oracle = {}


def oracle_of(c):
    """{task id: (node id or None, Err)} of ONE tick over the cluster, computed once per cluster."""
    if c.key not in _oracle:
        o = orc.Oracle()
        for d in c.nodes:
            o.create_node(d)
        for v in c.volumes:
            o.update_volume(v)
        for s in c.services:
            o.set_service(s)
        for t in c.tasks:
            o.create_task(t)
        _oracle[c.key] = {d["ID"]: ((d["NodeID"] or None) if d["State"] >= orc.ASSIGNED else None, d["Err"]) for d in o.tick()}
    return _oracle[c.key]


def engine_of(c, **engine_kw):
    """(host scheduler, descriptors): the cluster loaded, the tasks translated (one call per distinct task document, ID aside)."""
    s = swhost.HostScheduler(**engine_kw)
    for d in c.nodes:
        s.create_node(d)
    for v in c.volumes:
        s.update_volume(v)
    for sid in c.services:
        s.set_service(sid)
    seen, descs = {}, np.zeros(c.T, dtype=abi.TASK_DTYPE)
    for j, t in enumerate(c.tasks):
        k = json.dumps({a: b for a, b in t.items() if a != "ID"}, sort_keys=True)
        if k not in seen:
            seen[k] = s.task_desc(t)[0]
        descs[j] = seen[k]
    return s, descs


def all_rows(s, n):
    return s.e.node_get_many(np.arange(n, dtype=np.uint32)).tobytes() if n else b""


def run_plain(c):
    s, descs = engine_of(c)
    b = s.e.batch_prepare(descs)
    b.run()
    out, hist = b.fetch()
    att = b.attachments()
    res = dict(out=out, hist=hist, att=att, rows=all_rows(s, len(c.nodes)), stats=s.e.stats(), s=s)
    b.free()
    return res


def run_streamed(c, min_tasks=0, inside=None):
    s, descs = engine_of(c)
    b = s.e.batch_prepare(descs)
    calls = []

    def sink(first, nodes):
        calls.append((first, nodes.copy()))
        if inside:
            return inside(s, descs, calls)
    out = b.run_streamed(sink, min_tasks)
    _, hist = b.fetch()
    att = b.attachments()
    res = dict(out=out, hist=hist, att=att, rows=all_rows(s, len(c.nodes)), stats=s.e.stats(), calls=calls, s=s, descs=descs)
    b.free()
    return res


def check_ranges(c, calls, min_tasks):
    pos = 0
    for first, nodes in calls:
        assert first == pos and len(nodes) > 0, (first, pos)
        pos += len(nodes)
    assert pos == c.T
    assert all(len(n) >= max(min_tasks, 1) for _, n in calls[:-1]), [len(n) for _, n in calls]


def check_all(c, st, plain, min_tasks=0):
    """The four things every case is judged by."""
    check_ranges(c, st["calls"], min_tasks)
    seen = np.concatenate([n for _, n in st["calls"]]) if st["calls"] else np.zeros(0, dtype=np.int32)
    assert (seen == plain["out"]).all() and (st["out"] == plain["out"]).all()       # every range held the final answer
    want = oracle_of(c)
    s = st["s"]
    for j, t in enumerate(c.tasks):
        node, err = want[t["ID"]]
        got = s.idx_to_id[int(seen[j])] if seen[j] >= 0 else None
        assert got == node, (j, t["ID"], got, node)
        if node is None:
            ex = s.explain(st["hist"][j])
            assert err == ("no suitable node (" + ex + ")" if ex else "no suitable node"), (j, err, ex)
    assert (st["hist"] == plain["hist"]).all() and (st["att"] == plain["att"]).all()
    assert st["rows"] == plain["rows"]
    for k in ("batches", "tasks", "placed", "infeasible"):
        assert st["stats"][k] == plain["stats"][k], k


# ---- the clusters ----
def many_marks_cluster():
    return Cluster.of_workload("cfg3 2000x200x10", synth.Workload("cfg3", T=2000, N=200, services=10))


_plain = {}


def plain_of(c, env_key=""):
    """The plain run of a cluster on a twin engine, once per (cluster, knobs that change no result)."""
    if (c.key, env_key) not in _plain:
        _plain[(c.key, env_key)] = run_plain(c)
    return _plain[(c.key, env_key)]


# 1
def test_many_marks(monkeypatch):
    """Rounds of 64 tasks, a publish behind every fourth: the batch reaches the sink in many pieces, each final when it arrives. (The
    case the system-scope release in k_publish and the sentinel guard are for.)"""
    monkeypatch.setenv("SWP_R6_BLOCK", "64")
    monkeypatch.setenv("SWP_STREAM_EVERY", "4")
    c = many_marks_cluster()
    st = run_streamed(c, 0)
    print("sink calls:", [(f, len(n)) for f, n in st["calls"]])
    assert len(st["calls"]) >= 8
    assert st["calls"][0][0] == 0 and st["calls"][-1][0] + len(st["calls"][-1][1]) == c.T
    # Which of the marks lie behind ROUNDS: with ten services on 200 nodes the tasks soon have no plain candidates and a scan stretch takes
    # the rest of the batch, with one publish behind it. The ranges that end in front of the scanned tasks come from the publishes behind
    # every fourth round: the first chunk is 9 rounds (swp_rounds.hpp: 2000 / 256 rounded up + 1) = 3 publishes, and a stretch goes to the
    # scan resolver only after a further chunk of poor rounds = at least one more.
    by_rounds = [f + len(n) for f, n in st["calls"] if f + len(n) <= c.T - st["stats"]["scan_tasks"]]
    print("ranges behind rounds end at:", by_rounds, "scan tasks:", st["stats"]["scan_tasks"])
    assert len(by_rounds) >= 4
    check_all(c, st, plain_of(c))
    again = run_streamed(c, 0)   # min_tasks = 0: the sequence of calls is a function of the batch and the knobs
    assert [(f, len(n)) for f, n in again["calls"]] == [(f, len(n)) for f, n in st["calls"]]


# 2
def test_the_mirror_holds_a_range_when_the_sink_sees_it(monkeypatch):
    """The batch of test_many_marks with min_tasks = 300; the scan resolver off, so that the rounds carry the whole batch and the ranges
    are several (with it, one stretch takes everything behind task 212 and a minimum of 300 leaves one range)."""
    monkeypatch.setenv("SWP_R6_BLOCK", "64")
    monkeypatch.setenv("SWP_STREAM_EVERY", "4")
    monkeypatch.setenv("SWP_SCAN", "0")
    c = many_marks_cluster()
    s0, _ = engine_of(c)
    N = len(c.nodes)
    start = s0.e.node_get_many(np.arange(N, dtype=np.uint32))
    cpu, mem, total = start["cpu"].astype(np.int64).copy(), start["mem"].astype(np.int64).copy(), start["total"].astype(np.int64).copy()
    svc_count = {}
    checked = [0]

    def inside(s, descs, calls):
        first, nodes = calls[-1]
        for i, n in enumerate(nodes):   # the host replay of the ranges so far
            if n >= 0:
                d = descs[first + i]
                cpu[n] -= int(d["cpu"])
                mem[n] -= int(d["mem"])
                total[n] += 1
                svc_count[(int(n), int(d["service"]))] = svc_count.get((int(n), int(d["service"])), 0) + 1
        for i, n in enumerate(nodes):
            if n < 0:
                continue
            row = s.e.node_get(int(n))
            assert (row.cpu, row.mem, row.total) == (cpu[n], mem[n], total[n]), (first, int(n))
            svc = int(descs[first + i]["service"])
            assert s.e.node_get_svc_count(int(n), svc) == svc_count[(int(n), svc)]
            checked[0] += 1
        return False
    st = run_streamed(c, 300, inside)
    print("sink calls:", [(f, len(n)) for f, n in st["calls"]])
    assert checked[0] > 0 and len(st["calls"]) >= 2
    check_all(c, st, plain_of(c), 300)


# 3
@pytest.mark.parametrize("scan", ["default", "0"])
def test_scan_stretches(monkeypatch, scan):
    """A saturated small cluster: the rounds decide a handful of tasks each and the scan resolver takes stretches (a publish behind each);
    once more with the scan resolver switched off."""
    if scan == "0":
        monkeypatch.setenv("SWP_SCAN", "0")
    c = Cluster.of_workload("cfg2 1000x10x5", synth.Workload("cfg2", T=1000, N=10, services=5))
    st = run_streamed(c, 0)
    print("sink calls:", [(f, len(n)) for f, n in st["calls"]], "scan tasks:", st["stats"]["scan_tasks"])
    assert (st["stats"]["scan_tasks"] > 0) == (scan != "0")
    check_all(c, st, plain_of(c, scan))


# 4
def test_waterfill_runs(monkeypatch):
    """Service-major order: four runs of 500 identical tasks, each placed by one k_waterfill launch (SWP_WATERFILL=1: runs below the 512
    tasks that pay for a launch are taken too), a publish behind each."""
    monkeypatch.setenv("SWP_WATERFILL", "1")
    c = Cluster.of_workload("cfg3 major 2000x100x4", synth.Workload("cfg3", T=2000, N=100, services=4, order="major"))
    s, descs = engine_of(c)
    before = s.e.stats()["waterfill_tasks"]
    st = run_streamed(c, 0)
    print("sink calls:", [(f, len(n)) for f, n in st["calls"]], "waterfill tasks:", st["stats"]["waterfill_tasks"])
    assert st["stats"]["waterfill_tasks"] > before == 0
    assert len(st["calls"]) >= 2
    check_all(c, st, plain_of(c))


# 5
class MixedWorkload(synth.Workload):
    """cfg4's extras with more of them: a fifth of the services publish a host port, a third reserve generic resources, every seventh
    task is not counted on its node — none of which the bulk fold takes."""

    def __init__(self):
        super().__init__("cfg4", T=1500, N=150, services=30)
        self.svc_port = np.where(np.arange(self.S) % 5 == 0, 8000 + np.arange(self.S), 0)
        self.uncounted_every = 7

    def node_doc(self, i):
        d = super().node_doc(i)
        if i % 3 != 2:
            d["Description"]["Resources"]["Generic"] = [{"Discrete": {"Kind": "gpu", "Value": 1 + i % 4}}] + ([{"Discrete": {"Kind": "fpga", "Value": 2}}] if i % 2 else [])
        return d

    def service_spec(self, k):
        t = super().service_spec(k)
        if k % 3 == 1:
            t.setdefault("Spec", {}).setdefault("Resources", {}).setdefault("Reservations", {})["Generic"] = \
                [{"Discrete": {"Kind": "gpu", "Value": 1 + k % 2}}] + ([{"Discrete": {"Kind": "fpga", "Value": 1}}] if k % 2 else [])
        return t


def test_the_non_bulk_fold():
    wl = MixedWorkload()
    c = Cluster.of_workload("mixed 1500x150x30", wl)
    st = run_streamed(c, 0)
    plain = plain_of(c)
    d = st["descs"]
    assert (d["port_set"] != 0).any() and (d["generic_set"] != 0).any() and (d["flags"] & abi.TASK_UNCOUNTED).any()
    check_all(c, st, plain)
    kinds = [st["s"].e.intern(abi.SPACE_GENERIC_KIND, k) for k in ("gpu", "fpga")]
    for n in range(wl.N):   # the generic counts and the per-service counts are not part of a node row
        for k in kinds:
            assert st["s"].e.node_get_generic(n, k) == plain["s"].e.node_get_generic(n, k), (n, k)
    placed = st["out"] >= 0
    for j in np.flatnonzero(placed)[::7]:
        n, svc = int(st["out"][j]), int(d["service"][j])
        assert st["s"].e.node_get_svc_count(n, svc) == plain["s"].e.node_get_svc_count(n, svc)


# 6
def mounts_cluster():
    rng = random.Random(0x57E4)
    zones = ["z1", "z2", "z3"]
    nodes, vols, tasks = [], [], []
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
    for j in range(300):
        svc = "svc%d" % rng.randrange(4)
        if rng.random() < 0.5:
            mounts = [kv.cluster_mount(rng.choice(["name%02d" % rng.randrange(13), "group:" + rng.choice(["g1", "g2", "g9"])]), rng.choice(["/a", "/b", "/c"]), rng.random() < 0.4)
                      for _ in range(rng.choice([1, 1, 2, 3]))]
            t = sc.pending("t%05d" % j, svc, Spec={"Container": {"Mounts": mounts}})
        else:
            t = sc.pending("t%05d" % j, svc)
        if rng.random() < 0.5:
            t.setdefault("Spec", {})["Resources"] = {"Reservations": {"NanoCPUs": rng.choice([1, 2]) * 10**8, "MemoryBytes": 64 << 20}}
        tasks.append(t)
    return Cluster("mounts 300x40", nodes, ["svc%d" % k for k in range(4)], tasks, vols)


def test_cluster_mounts(monkeypatch):
    monkeypatch.setenv("SWP_R6_BLOCK", "64")
    monkeypatch.setenv("SWP_STREAM_EVERY", "1")
    c = mounts_cluster()
    st = run_streamed(c, 0)
    plain = plain_of(c)
    assert (st["att"] != abi.NO_VOLUME).any()          # some task got a volume: the attachments compared below are not all empty
    check_all(c, st, plain)
    for v in range(12):                                # the volumes' usage as the batch left it (what the engine holds per volume)
        assert st["s"].volume_info("vol%02d" % v)["Engine"] == plain["s"].volume_info("vol%02d" % v)["Engine"], v


# 7
def test_an_infeasible_tail():
    wl = synth.Workload("cfg2", T=500, N=30, services=8)
    huge = {"Resources": {"Reservations": {"NanoCPUs": 10**13, "MemoryBytes": 1 << 50}}}
    tail = [sc.pending("z%05d" % j, wl.service_id(j % 3), Spec=huge) for j in range(100)]
    c = Cluster.of_workload("cfg2 500x30 + 100 nobody holds", wl, tail)
    st = run_streamed(c, 0)
    seen = np.concatenate([n for _, n in st["calls"]])
    assert (seen[500:] == -1).all()                                   # -1 arrives in the stream ...
    assert (st["hist"][500:].sum(axis=1) == wl.N).all()               # ... and the histograms at fetch
    assert (st["hist"][500:, 1] > 0).all()                            # (insufficient resources)
    check_all(c, st, plain_of(c))


# 8
@pytest.mark.parametrize("T", [0, 1, 63, 64, 65])
def test_edge_sizes(monkeypatch, T):
    monkeypatch.setenv("SWP_R6_BLOCK", "64")
    monkeypatch.setenv("SWP_STREAM_EVERY", "1")
    c = Cluster.of_workload("cfg3 %dx50" % T, synth.Workload("cfg3", T=T, N=50, services=7))
    st = run_streamed(c, 0)
    if T == 0:
        assert st["calls"] == []
    check_all(c, st, plain_of(c))


def test_an_engine_without_nodes():
    wl = synth.Workload("cfg3", T=5, N=0, services=2)
    c = Cluster.of_workload("cfg3 5x0", wl)
    st = run_streamed(c, 0)
    assert [(f, list(n)) for f, n in st["calls"]] == [(0, [-1] * 5)]   # the empty nodeSet's answer, as one range
    check_all(c, st, plain_of(c))


# 9
def test_cancel_takes_everything_back(monkeypatch):
    monkeypatch.setenv("SWP_R6_BLOCK", "64")
    monkeypatch.setenv("SWP_STREAM_EVERY", "4")
    c = many_marks_cluster()
    s, descs = engine_of(c)
    N = len(c.nodes)
    before = all_rows(s, N)
    svc_before = [s.e.node_get_svc_count(n, int(descs["service"][0])) for n in range(N)]
    b = s.e.batch_prepare(descs)
    calls = []

    def sink(first, nodes):
        calls.append((first, len(nodes)))
        return len(calls) == 2
    with pytest.raises(abi.SwpError) as ei:
        b.run_streamed(sink, 0)
    assert ei.value.code == abi.SWP_ECANCELLED and len(calls) == 2
    assert all_rows(s, N) == before                                    # the first range left the mirror again
    assert [s.e.node_get_svc_count(n, int(descs["service"][0])) for n in range(N)] == svc_before
    with pytest.raises(abi.SwpError):
        b.fetch()                                                      # nothing to fetch: the run did not happen
    b.run()                                                            # the same batch, plainly, from the state as it was
    out, hist = b.fetch()
    b.free()
    plain = plain_of(c)
    assert (out == plain["out"]).all() and (hist == plain["hist"]).all() and all_rows(s, N) == plain["rows"]
    want = oracle_of(c)
    for j, t in enumerate(c.tasks):
        assert (s.idx_to_id[int(out[j])] if out[j] >= 0 else None) == want[t["ID"]][0], j


# 10
def test_a_shard_set_refuses():
    wl = synth.Workload("cfg3", T=100, N=40, services=5)
    s = swhost.HostScheduler(shards=2, nodes_per_shard=20)
    descs = swhost.load_workload(s, wl)
    out = np.full(wl.T, 12345, dtype=np.int32)
    called = []
    cb = abi.PREFIX_SINK(lambda ctx, first, count, nodes: called.append(first) or 0)
    rc = s.e.L.swp_schedule_batch_streamed(s.e.h, descs.ctypes.data, wl.T, out.ctypes.data, None, cb, None, 0)
    assert rc == abi.SWP_EUNSUPPORTED and not called and (out == 12345).all()
    b = s.e.batch_prepare(descs)
    rc = s.e.L.swp_batch_run_streamed(s.e.h, b.h, out.ctypes.data, cb, None, 0)
    assert rc == abi.SWP_EUNSUPPORTED and not called and (out == 12345).all()
    b.free()


# 11
def test_k_publish_ships_and_passes_the_kernel_checks():
    abi.build_library()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_kernels.py"), "--verbose"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    line = [l for l in r.stdout.splitlines() if " k_publish " in l]
    assert len(line) == 1, r.stdout
    assert " scratch    0 " in line[0] and "vgpr-spill 0" in line[0], line[0]
