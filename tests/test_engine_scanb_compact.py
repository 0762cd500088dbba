"""GPU: the BATCHED instance of the scan resolver on a compact stretch (csrc/swp_scan.hpp, k_scanb<.., true>): a labelled pool inside a
cluster of more nodes than one workgroup holds, saturated by services with more tasks than the pool has nodes. Where no task of the
stretch publishes host ports and the rows over the union fit in LDS (scan_lds_bc), four tasks share a barrier and the twins of an
unplaceable task are answered without a look; any other compact stretch keeps the one-task-a-barrier instance. Against the oracle,
decision for decision and Explain string for string; the counters scan_batched_tasks / scan_skipped of swp_stats say which ran.

The launcher takes the batched form by default for unions of at most 1 024 nodes (four nodes a thread); the pool of 1 208 nodes that
(a) - (f) use needs the eight-nodes-a-thread instance, which lost to the one-task kernel when it was measured, so those
tests ask for it with SWP_SCANB_COMPACT=1. (g) and (h) pin the default on both sides of the line.

Zone sizes of synth.Workload("cfg3") (asserted below): N = 5 000: z0 605 nodes, z1 603; N = 6 000: z0 .. z4 hold 3 680."""
import os
import re

import numpy as np
import pytest

import parity_util as pu
from swarmkit_amd import host as swhost
from swarmkit_amd import synth

pytestmark = pytest.mark.gpu

LDS_BUDGET = 160 * 1024 - 512


def scan_lds_bc(n_c, n_svc, n_sc):
    """csrc/swp_scan.hpp restated: node rows (24 bytes a node), the two (service, node) matrices, the class rows over the union; three
    sets of four argmins, the window's queue, its 256 records and descriptor ids, the table of 1 024 descriptors."""
    return ((n_c * 24 + 15) & ~15) + 2 * n_svc * n_c * 4 + n_sc * ((n_c + 63) // 64) * 8 + 3 * 4 * 8 + (256 // 64) * 8 + 16 + 256 * 64 + 256 * 4 + 1024 * 4


def pools(N, T, zones, order="rr"):
    """cfg3's cluster; len(zones) services, service k constrained to zone zones[k] and to nothing else."""
    wl = synth.Workload("cfg3", T=T, N=N, services=len(zones), order=order)
    wl.svc_zone = np.array(zones)
    wl.svc_nohdd = np.zeros(len(zones), dtype=bool)
    wl.svc_plat = np.zeros(len(zones), dtype=np.int64)
    return wl


def wl_a():
    return pools(5000, 6000, [0, 1, 0, 1])


def line(what, st):
    print(what + ":", " ".join("%s %d" % (k, st[k]) for k in ("scan_tasks", "scan_launches", "scan_batched_tasks", "scan_skipped")))


@pytest.fixture(scope="module")
def oracle_a():
    wl = wl_a()
    assert [int((wl.node_zone == z).sum()) for z in (0, 1)] == [605, 603]
    op, oe, _ = pu.oracle_run(wl)
    return op, oe


@pytest.fixture(scope="module")
def engine_a(oracle_a):
    old = os.environ.get("SWP_SCANB_COMPACT")
    os.environ["SWP_SCANB_COMPACT"] = "1"
    try:
        ep, ee, s, out, hist = pu.engine_run(wl_a())
    finally:
        if old is None:
            os.environ.pop("SWP_SCANB_COMPACT", None)
        else:
            os.environ["SWP_SCANB_COMPACT"] = old
    return ep, ee, s.e.stats(), out.copy()


@pytest.fixture
def batched(monkeypatch):
    monkeypatch.setenv("SWP_SCANB_COMPACT", "1")


def test_a_the_pools_dense_tail_goes_through_the_batched_instance(oracle_a, engine_a):
    """(a) four services of 1 500 tasks each for ~600 nodes, round-robin: 1 208 pool nodes, four services — ~90 KB of LDS."""
    op, oe = oracle_a
    ep, ee, st, _ = engine_a
    pu.assert_same(op, oe, ep, ee)
    line("(a)", st)
    assert scan_lds_bc(1208, 4, st["last_static_classes"]) <= LDS_BUDGET
    assert st["scan_batched_tasks"] > 0
    assert st["scan_tasks"] >= st["scan_batched_tasks"]


@pytest.mark.parametrize("knob,value,scanned", [("SWP_SCAN_UNBATCHED", "1", True), ("SWP_SCAN_COMPACT", "0", False)])
def test_b_without_the_batched_instance_the_same_answer(monkeypatch, batched, engine_a, knob, value, scanned):
    """(b) the one-task-a-barrier compact instance alone, and the rounds alone: the same placements and strings."""
    ep, ee, _, out = engine_a
    monkeypatch.setenv(knob, value)
    fp, fe, s, fout, _ = pu.engine_run(wl_a())
    pu.assert_same(ep, ee, fp, fe)
    assert (fout == out).all()
    st = s.e.stats()
    line("(b) %s=%s" % (knob, value), st)
    assert st["scan_batched_tasks"] == 0 and st["scan_skipped"] == 0
    assert (st["scan_tasks"] > 0) == scanned


def test_c_a_replica_limit_leaves_twins_nobody_looks_at(batched):
    """(c) MaxReplicas 2 on service 0, no ports: once a task of it found no node its twins are answered without a look; Explain is a pass
    over ALL nodes — those outside the union fail the constraint like the rest of the cluster outside the task's zone."""
    wl = wl_a()
    wl.svc_maxrep[0] = 2
    op, oe, _ = pu.oracle_run(wl)
    ep, ee, s, out, _ = pu.engine_run(wl)
    pu.assert_same(op, oe, ep, ee)
    st = s.e.stats()
    line("(c)", st)
    assert st["scan_batched_tasks"] > 0 and st["scan_skipped"] > 0
    left = sum(1 for j in range(0, wl.T, 4) if out[j] < 0)
    assert left == 1500 - 2 * 605
    outside_union = wl.N - int(np.isin(wl.node_zone, (0, 1)).sum())
    assert outside_union == 5000 - 1208
    j = next(j for j in range(0, wl.T, 4) if out[j] < 0)
    m = re.search(r"scheduling constraints not satisfied on (\d+) nodes", ee[wl.task_id(j)])
    assert m, ee[wl.task_id(j)]
    # (every node outside the union, and the rest of zone z1 but for the nodes an earlier filter of the pipeline refuses at that moment —
    # without a host port services 1 and 3 fill a few of z1's nodes up, and those count as short of resources. The string itself is the oracle's.)
    assert outside_union <= int(m.group(1)) <= wl.N - int((wl.node_zone == 0).sum())


def test_d_a_host_port_keeps_the_one_task_instance(batched):
    """(d) a host port on service 1, round-robin: every stretch names a task with ports, none is node-local."""
    wl = wl_a()
    wl.svc_port[1] = 8001
    op, oe, _ = pu.oracle_run(wl)
    ep, ee, s, *_ = pu.engine_run(wl)
    pu.assert_same(op, oe, ep, ee)
    st = s.e.stats()
    line("(d)", st)
    assert st["scan_tasks"] > 0 and st["scan_batched_tasks"] == 0 and st["scan_skipped"] == 0


def test_e_a_union_too_large_for_the_batched_instances_lds(batched):
    """(e) five services over zones z0 .. z4: 3 680 nodes fit the scan resolver's 4 096, their rows not k_scanb's LDS."""
    wl = pools(6000, 6000, [0, 1, 2, 3, 4])
    assert int(np.isin(wl.node_zone, range(5)).sum()) == 3680
    op, oe, _ = pu.oracle_run(wl)
    ep, ee, s, *_ = pu.engine_run(wl)
    pu.assert_same(op, oe, ep, ee)
    st = s.e.stats()
    line("(e)", st)
    assert scan_lds_bc(3680, 5, st["last_static_classes"]) > LDS_BUDGET
    assert st["scan_tasks"] > 0 and st["scan_batched_tasks"] == 0


def test_f_streamed(batched, engine_a):
    """(f) swp_schedule_batch_streamed on (a), min_tasks = 0: the ranges cover the batch once, put together they are the plain run's answer."""
    _, _, _, want = engine_a
    wl = wl_a()
    s = swhost.HostScheduler()
    descs = swhost.load_workload(s, wl)
    b = s.e.batch_prepare(descs)
    calls = []
    out = b.run_streamed(lambda first, nodes: calls.append((first, nodes.copy())), 0)
    st = s.e.stats()
    b.free()
    line("(f)", st)
    pos = 0
    for first, nodes in calls:
        assert first == pos and len(nodes) > 0, (first, pos)
        pos += len(nodes)
    assert pos == wl.T
    assert (np.concatenate([n for _, n in calls]) == want).all() and (out == want).all()
    assert st["scan_batched_tasks"] > 0


def test_g_a_pool_of_605_nodes_is_batched_by_default(monkeypatch):
    """(g) no knob: four services all on zone z0, 605 nodes — three a thread of the four-nodes-a-thread instance, which the launcher
    takes on its own. 6 000 tasks for 605 nodes whose services soon run everywhere."""
    monkeypatch.delenv("SWP_SCANB_COMPACT", raising=False)
    wl = pools(5000, 6000, [0, 0, 0, 0])
    assert int((wl.node_zone == 0).sum()) == 605
    op, oe, _ = pu.oracle_run(wl)
    ep, ee, s, *_ = pu.engine_run(wl)
    pu.assert_same(op, oe, ep, ee)
    st = s.e.stats()
    line("(g)", st)
    assert st["scan_batched_tasks"] > 0


def test_h_a_pool_of_1208_nodes_is_not_batched_by_default(monkeypatch, engine_a):
    """(h) no knob: (a)'s union is beyond 1 024 nodes — the one-task-a-barrier compact instance, the same answer."""
    monkeypatch.delenv("SWP_SCANB_COMPACT", raising=False)
    ep, ee, _, out = engine_a
    fp, fe, s, fout, _ = pu.engine_run(wl_a())
    pu.assert_same(ep, ee, fp, fe)
    assert (fout == out).all()
    st = s.e.stats()
    line("(h)", st)
    assert st["scan_tasks"] > 0 and st["scan_batched_tasks"] == 0
