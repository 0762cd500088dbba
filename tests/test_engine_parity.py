"""GPU parity: HIP engine (through the C ABI) vs the CPU oracle on identical seeded inputs — bit-exact
placements and identical 'no suitable node (...)' explanations."""
import numpy as np
import pytest

import parity_util as pu
from swarmkit_amd import abi, synth

pytestmark = pytest.mark.gpu


def test_abi_roundtrip():
    e = abi.Engine()
    e.reset(4)
    n0 = e.intern(abi.SPACE_NODE_ID, "a")
    n1 = e.intern(abi.SPACE_NODE_ID, "b")
    assert (n0, n1) == (0, 1) and e.intern(abi.SPACE_NODE_ID, "a") == 0
    assert e.intern(abi.SPACE_FOLDED, "SSD") == e.intern(abi.SPACE_FOLDED, "ssd")
    assert e.intern(abi.SPACE_ARCH, "x86_64") == e.intern(abi.SPACE_ARCH, "amd64")
    row = abi.NodeRow(node=n1, flags=abi.NODE_READY, cpu=5, mem=7, total=3)
    e.node_upsert(row)
    got = e.node_get(n1)
    assert (got.cpu, got.mem, got.total) == (5, 7, 3)
    assert e.node_get(n0) is None   # errNodeNotFound
    e.node_remove(n1)
    assert e.node_get(n1) is None


def test_service_counts_of_a_service_id_beyond_the_dense_index():
    """The engine's service -> nodes index is a vector by service id up to 2^20 ids and a map beyond (swp_engine.hip SvcNodes): counts set,
    changed by swp_commit and dropped with the node behave the same on both sides of that border."""
    e = abi.Engine()
    e.reset(4)
    nodes = [e.intern(abi.SPACE_NODE_ID, "n%d" % i) for i in range(3)]
    for n in nodes:
        e.node_upsert(abi.NodeRow(node=n, flags=abi.NODE_READY, cpu=100, mem=100, total=0))
    for svc in (5, (1 << 20) - 1, 1 << 20, 3_000_000_000):
        e.node_set_svc_count(nodes[0], svc, 7)
        e.node_set_svc_count(nodes[2], svc, 1)
        assert [e.node_get_svc_count(n, svc) for n in nodes] == [7, 0, 1]
        pl = np.zeros(2, dtype=abi.PLACEMENT_DTYPE)
        pl["node"], pl["service"], pl["cpu"], pl["mem"], pl["counted"] = [nodes[1], nodes[2]], svc, 1, 1, 1
        e.commit(pl, add=True)
        assert [e.node_get_svc_count(n, svc) for n in nodes] == [7, 1, 2]
        e.commit(pl, add=False)
        assert [e.node_get_svc_count(n, svc) for n in nodes] == [7, 0, 1]
        e.node_set_svc_count(nodes[2], svc, 0)
        assert e.node_get_svc_count(nodes[2], svc) == 0
    e.node_remove(nodes[0])
    n0 = e.intern(abi.SPACE_NODE_ID, "again")   # the lowest free index: the removed node's
    assert n0 == nodes[0]
    e.node_upsert(abi.NodeRow(node=n0, flags=abi.NODE_READY, cpu=100, mem=100, total=0))
    assert [e.node_get_svc_count(n0, svc) for svc in (5, 1 << 20, 3_000_000_000)] == [0, 0, 0]


@pytest.mark.parametrize("name,T,N", [("cfg2", 2000, 300), ("cfg2", 10_000, 1_000), ("cfg3", 6000, 1000), ("cfg4", 6000, 1500)])
def test_parity_one_off(name, T, N):
    wl = synth.Workload(name, T=T, N=N)
    op, oe, _ = pu.oracle_run(wl)
    ep, ee, s, out, hist = pu.engine_run(wl)
    pu.assert_same(op, oe, ep, ee)
    # the host mirror folded the placements: counts agree with the oracle's nodeSet
    st = s.e.stats()
    assert st["placed"] == sum(v is not None for v in op.values())


@pytest.mark.parametrize("block", [64, 256, 1024])
def test_parity_block_sizes(block, monkeypatch):
    """Result must not depend on how many tasks a round of the block resolver takes (SWP_R6_BLOCK: the freshness of the candidate lists)."""
    monkeypatch.setenv("SWP_R6_BLOCK", str(block))
    wl = synth.Workload("cfg3", T=3000, N=500)
    op, oe, _ = pu.oracle_run(wl)
    ep, ee, *_ = pu.engine_run(wl)
    pu.assert_same(op, oe, ep, ee)


def test_parity_tight_capacity():
    """Nodes fill up inside the batch: exercises the touched-node re-check and the explain pass."""
    wl = synth.Workload("cfg2", T=4000, N=60)
    op, oe, _ = pu.oracle_run(wl)
    assert any(v is None for v in op.values())
    ep, ee, *_ = pu.engine_run(wl)
    pu.assert_same(op, oe, ep, ee)


def test_parity_single_service():
    """All tasks of ONE service (the shape of the reference's own benchScheduler): every node becomes an
    exception node after the first round, so the slow path carries the batch."""
    wl = synth.Workload("cfg1", T=700, N=40)
    op, oe, _ = pu.oracle_run(wl)
    ep, ee, *_ = pu.engine_run(wl)
    pu.assert_same(op, oe, ep, ee)


def test_second_batch_sees_first():
    wl = synth.Workload("cfg3", T=2000, N=400)
    o = None
    op1, oe1, o = pu.oracle_run(wl, count=1000)
    for j in range(1000, 2000):
        o.create_task(wl.task_doc(j))
    second = {d["ID"]: (d["NodeID"] or None) for d in o.tick() if d["ID"] >= wl.task_id(1000)}
    from swarmkit_amd import host as swhost
    s = swhost.HostScheduler()
    descs = swhost.load_workload(s, wl)
    out1, _ = s.e.schedule_batch(descs[:1000])
    out2, _ = s.e.schedule_batch(descs[1000:2000])
    for j in range(1000, 2000):
        want = second.get(wl.task_id(j))
        got = s.idx_to_id[int(out2[j - 1000])] if out2[j - 1000] >= 0 else None
        if want is not None or wl.task_id(j) in second:
            assert want == got, (j, want, got)


@pytest.mark.parametrize("name", ["cfg2_small", "cfg3_small", "cfg4_small"])
def test_engine_matches_golden_fixture(name):
    import json
    import os
    g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".json")))
    wl = synth.Workload(g["workload"], T=g["T"], N=g["N"])
    ep, ee, *_ = pu.engine_run(wl)
    assert [ep[wl.task_id(j)] for j in range(wl.T)] == g["node_of_task"]
    assert ee == g["errors"]


def test_every_resolver_variant_is_exact():
    """the block resolver must give the oracle's placements."""
    wl = synth.Workload("cfg4", T=4000, N=700)
    op, oe, _ = pu.oracle_run(wl)
    ep, ee, *_ = pu.engine_run(wl)
    pu.assert_same(op, oe, ep, ee)


def test_full_size_properties():
    """BASELINE shape (100k x 10k): size-independent properties instead of a full oracle run —
    every placement is feasible for its task on final accounting, per-node resources never go negative
    beyond the initial state, counts add up, and a prefix agrees with the oracle bit for bit."""
    wl = synth.Workload("cfg3")
    from swarmkit_amd import host as swhost
    s = swhost.HostScheduler()
    descs = swhost.load_workload(s, wl)
    out, hist = s.e.schedule_batch(descs)
    placed = out >= 0
    assert placed.sum() + (~placed).sum() == wl.T
    # residual accounting: cpu/mem used per node == sum of reservations of the tasks placed there
    svc = np.arange(wl.T) % wl.S
    used_cpu = np.bincount(out[placed], weights=wl.svc_cpu[svc][placed].astype(np.float64), minlength=wl.N)
    used_mem = np.bincount(out[placed], weights=wl.svc_mem[svc][placed].astype(np.float64), minlength=wl.N)
    assert (used_cpu <= wl.node_cpu).all() and (used_mem <= wl.node_mem).all()
    for n in (0, 17, wl.N - 1):
        row = s.e.node_get(n)
        assert row.cpu == int(wl.node_cpu[n]) - int(used_cpu[n]) and row.mem == int(wl.node_mem[n]) - int(used_mem[n])
        assert row.total == int((out == n).sum())
    # constraint / platform feasibility of every placement, recomputed on the host from the raw tables
    zone_ok = (wl.svc_zone[svc] < 0) | (wl.svc_zone[svc] == wl.node_zone[np.clip(out, 0, None)])
    disk_ok = ~wl.svc_nohdd[svc] | wl.node_ssd[np.clip(out, 0, None)]
    arch = np.where(np.isin(wl.node_arch, ["x86_64", "amd64"]), "amd64", "arm64")[np.clip(out, 0, None)]
    os_ = wl.node_os[np.clip(out, 0, None)]
    plat = wl.svc_plat[svc]
    plat_ok = (plat == 0) | ((os_ == "linux") & ((arch == "amd64") | ((plat == 2) & (arch == "arm64"))))
    assert (zone_ok & disk_ok & plat_ok)[placed].all()
    # unplaceable tasks explain themselves over all N nodes
    assert (hist[~placed].sum(axis=1) == wl.N).all()
    # spread: no service has two tasks on one node while it had an empty feasible node ... checked on a prefix vs the oracle
    n = 2500
    op, oe, _ = pu.oracle_run(wl, count=n)
    for j in range(n):
        want = op[wl.task_id(j)]
        got = s.idx_to_id[int(out[j])] if out[j] >= 0 else None
        assert want == got, (j, want, got)
