"""GPU: dense stretches on a cluster of more nodes than the scan resolver's one workgroup holds (4 096). Services constrained to a
labelled pool, with more tasks than the pool has nodes: every node of the pool soon runs its services and each task has to take the
best node of its service's exception list. The union of such a stretch's static class rows is the pool, so the stretch goes through the
COMPACT instance of the scan resolver (csrc/swp_scan.hpp); where the union is wider than 4 096 nodes the probe refuses and the rounds of
the block resolver carry on. Against the oracle, decision for decision and Explain string for string; SWP_SCAN_COMPACT=0 / SWP_SCAN=0
(the rounds alone, as before the instance existed) must give the same answer.

Zone sizes of synth.Workload("cfg3") (asserted below): N = 5 000: z0 605 nodes, z1 603; N = 6 000: z0 .. z5 hold 4 431."""
import re

import numpy as np
import pytest

import parity_util as pu
from swarmkit_amd import host as swhost
from swarmkit_amd import synth

pytestmark = pytest.mark.gpu


def pools(N, T, zones, order="rr"):
    """cfg3's cluster; len(zones) services, service k constrained to zone zones[k] and to nothing else."""
    wl = synth.Workload("cfg3", T=T, N=N, services=len(zones), order=order)
    wl.svc_zone = np.array(zones)
    wl.svc_nohdd = np.zeros(len(zones), dtype=bool)
    wl.svc_plat = np.zeros(len(zones), dtype=np.int64)
    return wl


def wl_a(order="rr"):
    return pools(5000, 6000, [0, 1, 0, 1], order)


@pytest.fixture(scope="module")
def oracle_a():
    wl = wl_a()
    assert [int((wl.node_zone == z).sum()) for z in (0, 1)] == [605, 603]
    op, oe, _ = pu.oracle_run(wl)
    return op, oe


@pytest.fixture(scope="module")
def engine_a(oracle_a):
    ep, ee, s, out, hist = pu.engine_run(wl_a())
    return ep, ee, s.e.stats(), out.copy()


def test_a_pool_of_1208_nodes_in_5000_goes_through_the_compact_scan(oracle_a, engine_a):
    """(a) four services of 1 500 tasks each for ~600 nodes, round-robin: the dense tail is scanned (never, before the instance existed:
    5 000 nodes are more than the scan resolver takes)."""
    op, oe = oracle_a
    ep, ee, st, _ = engine_a
    pu.assert_same(op, oe, ep, ee)
    print("scan_tasks", st["scan_tasks"], "scan_launches", st["scan_launches"])
    assert st["scan_tasks"] > 0


@pytest.mark.parametrize("knob", ["SWP_SCAN_COMPACT", "SWP_SCAN"])
def test_b_the_rounds_alone_give_the_same_answer(monkeypatch, engine_a, knob):
    """(b) the same batch with the instance switched off: the same placements and strings, nothing scanned."""
    ep, ee, _, out = engine_a
    monkeypatch.setenv(knob, "0")
    fp, fe, s, fout, _ = pu.engine_run(wl_a())
    pu.assert_same(ep, ee, fp, fe)
    assert (fout == out).all()
    assert s.e.stats()["scan_tasks"] == 0


def test_c_service_major_one_zone_at_a_time(monkeypatch):
    """(c) service-major: the union is one zone at a time, and the rounds take over between the services. As the batch stands, its four
    runs of 1 500 identical tasks are water-filled (k_waterfill, csrc/swp_waterfill.hpp) and no round is ever run — scan_launches 0 on
    the first GPU run of this test —, so the stretches are checked with SWP_WATERFILL=0, where the rounds carry the runs; the batch as
    it stands must match the oracle as well."""
    wl = wl_a("major")
    op, oe, _ = pu.oracle_run(wl)
    ep, ee, s, *_ = pu.engine_run(wl)
    pu.assert_same(op, oe, ep, ee)
    st = s.e.stats()
    print("water-filled: scan_tasks", st["scan_tasks"], "scan_launches", st["scan_launches"], "waterfill_tasks", st["waterfill_tasks"])
    monkeypatch.setenv("SWP_WATERFILL", "0")
    ep, ee, s, *_ = pu.engine_run(wl)
    pu.assert_same(op, oe, ep, ee)
    st = s.e.stats()
    print("by rounds: scan_tasks", st["scan_tasks"], "scan_launches", st["scan_launches"])
    assert st["scan_launches"] >= 2


def test_d_unplaceable_tasks_count_the_nodes_outside_the_union():
    """(d) MaxReplicas 2 on service 0 (~290 tasks find no node) and a host port on service 1 (~900): Explain is a pass over ALL nodes —
    the ~3 800 outside the union fail the constraint like the rest of the cluster outside the task's own zone."""
    wl = wl_a()
    wl.svc_maxrep[0] = 2
    wl.svc_port[1] = 8001
    op, oe, _ = pu.oracle_run(wl)
    ep, ee, s, out, _ = pu.engine_run(wl)
    pu.assert_same(op, oe, ep, ee)
    assert s.e.stats()["scan_tasks"] > 0
    left = [sum(1 for j in range(k, wl.T, 4) if out[j] < 0) for k in (0, 1)]
    print("unplaceable tasks of services 0 and 1:", left)
    assert left == [1500 - 2 * 605, 1500 - 603]
    outside_union = wl.N - int(np.isin(wl.node_zone, (0, 1)).sum())
    assert outside_union == 5000 - 1208
    for k in (0, 1):
        j = next(j for j in range(k, wl.T, 4) if out[j] < 0)
        m = re.search(r"scheduling constraints not satisfied on (\d+) nodes", ee[wl.task_id(j)])
        assert m, ee[wl.task_id(j)]
        assert int(m.group(1)) == wl.N - int((wl.node_zone == k).sum()) >= outside_union


def test_e_a_union_wider_than_4096_nodes_is_refused():
    """(e) six services over zones z0 .. z5, round-robin: every stretch the driver can form names all six pools, 4 431 nodes."""
    wl = pools(6000, 6000, [0, 1, 2, 3, 4, 5])
    assert int(np.isin(wl.node_zone, range(6)).sum()) == 4431
    op, oe, _ = pu.oracle_run(wl)
    ep, ee, s, *_ = pu.engine_run(wl)
    pu.assert_same(op, oe, ep, ee)
    assert s.e.stats()["scan_tasks"] == 0


def test_f_streamed(engine_a):
    """(f) swp_schedule_batch_streamed on (a), min_tasks = 0: the ranges cover the batch once, put together they are the plain run's answer
    (the probe's word comes back through the pinned words, the publishes go on behind every stretch)."""
    _, _, _, want = engine_a
    wl = wl_a()
    s = swhost.HostScheduler()
    descs = swhost.load_workload(s, wl)
    b = s.e.batch_prepare(descs)
    calls = []
    out = b.run_streamed(lambda first, nodes: calls.append((first, nodes.copy())), 0)
    st = s.e.stats()
    b.free()
    pos = 0
    for first, nodes in calls:
        assert first == pos and len(nodes) > 0, (first, pos)
        pos += len(nodes)
    assert pos == wl.T
    assert (np.concatenate([n for _, n in calls]) == want).all() and (out == want).all()
    assert st["scan_tasks"] > 0
