"""GPU: a compact spread segment whose class rows' union is too wide is CUT at the preparation instead of refusing the batch
(csrc/swp_scan_spread.hpp k_spread_cut, csrc/swp_engine.hip spread_cut) — an unconstrained plain task riding along between tasks with
preferences that are constrained to a pool, two pools that fit one by one and not together — against the oracle (tests/orc.py),
decision for decision, "no suitable node (...)" strings included.

The driver, the comparison and the helpers are those of tests/test_engine_oneoff_spread.py and tests/test_engine_oneoff_spread_compact.py
(WholeRun: a tick's one-off tasks go down as ONE batch, no host split; afterwards every node's row and per-service counts are compared,
and a second tick runs on that state). 4 200 node slots, at most 400 tasks. On the parent commit every such batch but those of `fits`
and `own_row` is refused with SWP_EUNSUPPORTED ("... the union of the class rows of segment ...").

The CPU side of the kernel — its source on fibers against a bitset model of the rule — is tests/test_emu_spread_cut.py."""
import os
import random

import numpy as np
import pytest

import orc
import scenarios as sc
from swarmkit_amd import abi
from swarmkit_amd import host as swhost
from test_engine_oneoff_spread import MIB, WholeRun, key, node, oracle_of, run_script, running, spread
from test_engine_oneoff_spread_compact import all_rows, first_tick, loaded, placements, pool_nodes, pooled

pytestmark = pytest.mark.gpu
N = 4200
ZONES = 5
LIMIT = 4096   # (the trees of these scripts are small: the spread kernel's LDS holds the rows of 4 096 nodes next to them)


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    for k in ("SWP_R6_BLOCK", "SWP_STREAM_EVERY", "SWP_SCAN", "SWP_WATERFILL", "SWP_SCHED_ONEOFF_SPREAD", "SWP_HOST", "SWP_SCANB_COMPACT", "SWP_SCAN_UNBATCHED"):
        monkeypatch.delenv(k, raising=False)


# ------------------------------------------------------------------------------------------------------------------ the shapes
def riders_tasks(runs=44, group=False):
    """Runs of 5 tasks with preferences constrained to the pool, 1 to 3 unconstrained plain tasks between two runs.
    -> (events, spread runs, plain gaps, tasks with preferences)"""
    ev, at, gaps = [], 0, 0
    res = {"Resources": {"Reservations": {"MemoryBytes": 200 * MIB}}}
    for r in range(runs):
        for j in range(5):
            ev.append(("create_task", pooled("t%04d" % at, "ab"[(r + j) % 2], mem=300 if j % 2 else 0)))
            at += 1
        if r + 1 < runs:
            for j in range(1 + r % 3):
                ev.append(("create_task", sc.pending("t%04d" % at, "c", Spec=res)))
                at += 1
            gaps += 1
    assert at <= 400
    return ev, runs, gaps, runs * 5


def shape_riders():
    """A pool every 14th node carries (300 of 4 200). The segment's union with a rider in it is the whole nodeSet."""
    ev = pool_nodes() + [("set_service", "a"), ("set_service", "b"), ("set_service", "c")]
    return ev + riders_tasks()[0] + [("tick",), ("create_task", pooled("u0", "a")), ("create_task", sc.pending("u1", "c")), ("create_task", pooled("u2", "b")), ("tick",)]


def wide_nodes(split=None):
    """Two pools: the even and the odd nodes (2 100 each), or with `split` the nodes below it and the others."""
    return [("create_node", node(i, {"zone": "z%d" % (i * 7 % ZONES), "pool": "a" if (i % 2 == 0 if split is None else i < split) else "b"}, mem_gib=1 + i % 2)) for i in range(N)]


WIDE_BLOCKS = 16


def shape_wide_pools(split=None):
    """Blocks of 20 tasks with preferences, alternating between the two pools, no plain task between them: each pool fits, their union
    (all 4 200 nodes) does not."""
    ev = wide_nodes(split) + [("set_service", "a"), ("set_service", "b")]
    for k in range(WIDE_BLOCKS):
        for j in range(20):
            ev.append(("create_task", pooled("t%04d" % (k * 20 + j), "ab"[j % 2], "ab"[k % 2], mem=700 if j % 3 == 0 else 0)))
    return ev + [("tick",), ("create_task", pooled("u0", "a", "b")), ("create_task", pooled("u1", "a", "a")), ("tick",)]


def shape_fits():
    """Pools of 300 and 200 in ONE segment, a plain rider constrained to the pool between them: a union of 500, nothing is cut."""
    ev = pool_nodes(pools=(("a", 14, 0), ("b", 21, 5))) + [("set_service", "a"), ("set_service", "b")]
    for k in range(6):
        for j in range(15):
            ev.append(("create_task", pooled("t%04d" % (k * 20 + j), "ab"[j % 2], "ab"[k % 2], mem=300 if j % 2 else 0)))
        for j in range(15, 18):
            ev.append(("create_task", pooled("t%04d" % (k * 20 + j), "a", "ab"[k % 2], prefs=())))
    return ev + [("tick",), ("tick",)]


def big_pref(tid):
    return sc.pending(tid, "b", Spec={"Placement": {"Constraints": ["node.labels.big==1"], "Preferences": spread("node.labels.zone")}})


def shape_own_row():
    """A task with preferences constrained to a pool of 4 097 nodes between tasks constrained to the pool of 300."""
    ev = []
    for i in range(N):
        labels = {"zone": "z%d" % (i * 7 % ZONES)}
        if i % 14 == 0:
            labels["pool"] = "a"
        if i < 4097:
            labels["big"] = "1"
        ev.append(("create_node", node(i, labels, mem_gib=1)))
    ev += [("set_service", "a"), ("set_service", "b")]
    for j in range(5):
        ev.append(("create_task", pooled("t%04d" % j, "a")))
    ev.append(("create_task", big_pref("t0005")))
    for j in range(6, 11):
        ev.append(("create_task", pooled("t%04d" % j, "a")))
    return ev + [("tick",)]


SHAPES = {"riders": shape_riders, "wide_pools": shape_wide_pools, "fits": shape_fits}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_one_batch_against_the_oracle(name):
    e = run_script("cut_" + name, SHAPES[name]())
    assert e.calls == (1 if name == "fits" else 2)   # (a batch a tick; the second tick of `fits` has no task)


def test_riders_has_a_segment_per_run_and_rounds_between():
    _, runs, gaps, _ = riders_tasks()
    st = first_tick(shape_riders()).e.stats()
    assert runs == 44 and gaps == 43
    assert st["resolve_launches"] > 0, st          # the riders: rounds of the block resolver (their union is the whole nodeSet)
    assert st["scan_launches"] >= runs, st         # a spread segment per run (counted with the scan stretches)


def test_wide_pools_has_a_segment_per_block():
    st = first_tick(shape_wide_pools()).e.stats()
    assert st["scan_launches"] >= WIDE_BLOCKS and st["scan_tasks"] == WIDE_BLOCKS * 20, st


@pytest.mark.parametrize("mode", ["prepared", "templates", "streamed"])
@pytest.mark.parametrize("name", ["riders", "wide_pools"])
def test_prepared_and_streamed_entries(name, mode):
    e = run_script("cut_" + name, SHAPES[name](), mode)
    if mode == "streamed":   # (WholeRun asserts that the ranges tile [0, T))
        assert e.ranges and e.ranges[0] >= 3, e.ranges


# ------------------------------------------------------------------------------------------------------------------ limits
def test_an_own_row_of_4097_is_refused():
    e, descs = loaded(shape_own_row())
    rows = all_rows(e)
    for call in (e.e.schedule_batch, e.e.batch_prepare, lambda d: e.e.schedule_batch_streamed(d, lambda *a: False)):
        with pytest.raises(abi.SwpError) as err:
            call(descs)
        assert err.value.code == abi.SWP_EUNSUPPORTED and "4096" in str(err.value) and "swp_schedule_groups" in str(err.value)
        assert "segment 0, tasks [0, 11)" in str(err.value)   # (the segment as spread_segments made it, not a piece)
    assert all_rows(e) == rows
    plain_task = e.task_desc(sc.pending("plain", "a"))   # (and the engine goes on)
    out, _ = e.e.schedule_batch(plain_task)
    assert out[0] >= 0


def test_a_label_that_moves_between_prepare_and_run():
    """Prepared on wide_pools with pools of 4 096 and 104: the pieces of pool a have a union of exactly 4 096. One node of pool b is
    labelled into pool a: the run does not cut again, it is refused, rows unchanged. The label taken back, a fresh preparation runs."""
    ev = shape_wide_pools(split=4096)
    ev = ev[:ev.index(("tick",)) + 1]
    e, descs = loaded(ev)
    b = e.e.batch_prepare(descs)
    e.create_node(node(4096, {"zone": "z%d" % (4096 * 7 % ZONES), "pool": "a"}, mem_gib=1))
    rows = all_rows(e)
    with pytest.raises(abi.SwpError) as err:
        b.run()
    assert err.value.code == abi.SWP_EUNSUPPORTED and "4096" in str(err.value) and "4097" in str(err.value)
    assert all_rows(e) == rows
    b.free()
    e.create_node(node(4096, {"zone": "z%d" % (4096 * 7 % ZONES), "pool": "b"}, mem_gib=1))
    b = e.e.batch_prepare(descs)
    b.run()
    out, _ = b.fetch()
    b.free()
    want, _ = oracle_of("cut_wide_pools_4096", ev)
    ids = [tid for tid, _ in e.unassigned.items()]
    assert {tid: ("n%05d" % n if n >= 0 else "") for tid, n in zip(ids, out)} == placements(want)


# ------------------------------------------------------------------------------------------------------------------ the rule, restated
SPREAD_GAP = 64


def spread_segments(prefs):
    """csrc/swp_rounds.hpp spread_segments for a batch without fences: [(first, count, spread)]."""
    out, plain0, j, T = [], 0, 0, len(prefs)
    while j < T:
        if not prefs[j]:
            j += 1
            continue
        end, gap = j + 1, 0
        for k in range(j + 1, T):
            if prefs[k]:
                end, gap = k + 1, 0
                continue
            gap += 1
            if gap >= SPREAD_GAP:
                break
            if k + 1 == T:
                end = T
        if j > plain0:
            out.append((plain0, j - plain0, 0))
        out.append((j, end - j, 1))
        plain0 = j = end
    if T > plain0:
        out.append((plain0, T - plain0, 0))
    return out


def popc(x):
    return bin(x).count("1")


def cut_facts(rows, prefs, limit=LIMIT):
    """The rule of k_spread_cut on a tick's tasks (rows: a bit mask of nodes per task): (segments too wide, cuts at a plain task, cuts
    at a task with preferences, own rows too wide)."""
    wide = at_plain = at_pref = own = 0
    for j0, n, is_spread in spread_segments(prefs):
        if not is_spread:
            continue
        j1, u = j0 + n, 0
        for t in range(j0, j1):
            u |= rows[t]
        if popc(u) <= limit:
            continue
        wide += 1
        j = j0
        while j < j1:
            u = rows[j]
            if popc(u) > limit:
                own += 1
                break
            k = j + 1
            while k < j1 and popc(u | rows[k]) <= limit:
                u |= rows[k]
                k += 1
            if k == j1:
                break
            if prefs[k]:
                at_pref += 1
                j = k
            else:
                at_plain += 1
                j = k + 1
                while j < j1 and not prefs[j]:
                    j += 1
    return wide, at_plain, at_pref, own


def test_the_restated_rule_on_the_shapes():
    """(CPU: the scripts alone.) riders: a cut at a plain task per gap; wide_pools: a cut at a task with preferences per block boundary;
    fits: none; own_row: the own row."""
    pool = sum(1 << i for i in range(N) if i % 14 == 0)
    everything = (1 << N) - 1
    _, runs, gaps, _ = riders_tasks()
    rows, prefs = [], []
    for r in range(runs):
        rows += [pool] * 5
        prefs += [1] * 5
        if r + 1 < runs:
            rows += [everything] * (1 + r % 3)
            prefs += [0] * (1 + r % 3)
    assert cut_facts(rows, prefs) == (1, gaps, 0, 0)
    even = sum(1 << i for i in range(0, N, 2))
    rows = sum(([even if k % 2 == 0 else everything ^ even] * 20 for k in range(WIDE_BLOCKS)), [])
    assert cut_facts(rows, [1] * len(rows)) == (1, 0, WIDE_BLOCKS - 1, 0)
    b = sum(1 << i for i in range(N) if i % 21 == 5)
    assert cut_facts([pool] * 15 + [b] * 15, [1] * 14 + [0] + [1] * 15) == (0, 0, 0, 0)
    big = (1 << 4097) - 1
    assert cut_facts([pool] * 5 + [big] + [pool] * 5, [1] * 11) == (1, 0, 1, 1)


# ------------------------------------------------------------------------------------------------------------------ fuzz
KEYS = ["zone", "rack", "tier"]


def fuzz_script(seed):
    """(events, facts): 4 097 - 4 400 nodes; two or three pools of 50 - 2 500 nodes (a label key each; the first two disjoint, in half
    of the seeds with more than 4 096 nodes between them); services with 1 - 3 spread levels constrained to one pool, plain services
    constrained to a pool or to nothing; runs of 1 - 30 tasks with preferences with gaps of 1 - 80 plain tasks between them, at most
    400 tasks over two ticks; nodes that are not ready, services that run already inside and outside their pool, reservations tight
    enough that tasks stay unplaced, MaxReplicas. facts: per tick the rule's (wide segments, cuts at a plain task, cuts at a task with
    preferences, own rows) from the labels alone."""
    rng = random.Random(0xC07 + seed)
    n_nodes = rng.randrange(4097, 4401)
    n_keys = rng.choice([2, 3])
    vals = [rng.randrange(1, 6) for _ in range(n_keys)]
    n_pools = rng.choice([2, 3])
    down = set(rng.sample(range(n_nodes), rng.randrange(0, min(60, n_nodes - 4097) + 1)))   # nodes that are not ready
    order = [i for i in range(n_nodes) if i not in down]
    rng.shuffle(order)
    if seed % 2 == 0:   # the first two pools (ready nodes) do not fit together
        size_a = rng.randrange(1700, 2501)
        size_b = rng.randrange(4097 - size_a, min(2500, len(order) - size_a) + 1)
    else:
        size_a, size_b = rng.choice([50, 300, 1000, 2500]), rng.choice([50, 200, 1500])
    members = [set(order[:size_a]), set(order[size_a:size_a + size_b])]
    if n_pools == 3:
        members.append(set(rng.sample(range(n_nodes), rng.choice([50, 400, 2500]))))
    ev, ready_mask = [], 0
    for i in range(n_nodes):
        labels = {}
        for k in range(n_keys):
            if rng.random() < 0.9:
                labels[KEYS[k]] = "v%d" % rng.randrange(vals[k])
        for p in range(n_pools):
            if i in members[p]:
                labels["pool%d" % p] = "1"
        ready = i not in down
        ready_mask |= int(ready) << i
        ev.append(("create_node", node(i, labels, cpu=rng.choice([2, 4, 8]), mem_gib=rng.choice([1, 2, 4]), ready=ready)))
    pool_mask = [sum(1 << i for i in m) & ready_mask for m in members]
    n_spread, n_plain = rng.randrange(2 if seed % 2 == 0 else 1, 5), rng.randrange(1, 4)
    rider = 0.15 if seed % 2 == 0 else 0.4   # how many plain services are constrained to nothing (the riders)
    specs, masks = [], []   # services 0 .. n_spread - 1 have preferences
    for s in range(n_spread + n_plain):
        ev.append(("set_service", "svc%d" % s))
        pl, spec = {}, {}
        pool = rng.randrange(n_pools) if s < n_spread or rng.random() >= rider else None
        if s < n_spread and seed % 2 == 0:
            pool = s % 2 if s < 2 else pool
        if pool is not None:
            pl["Constraints"] = ["node.labels.pool%d==1" % pool]
        if s < n_spread:
            pl["Preferences"] = spread(*["node.labels." + KEYS[k] for k in rng.sample(range(n_keys), rng.randrange(1, n_keys + 1))])
        if rng.random() < 0.2:
            pl["MaxReplicas"] = rng.choice([1, 2, 3])
        if rng.random() < 0.7:
            spec["Resources"] = {"Reservations": {"NanoCPUs": rng.choice([0, 500, 1000, 2000]) * 10**6, "MemoryBytes": rng.choice([0, 256, 700, 1500]) * MIB}}
        spec["Placement"] = pl
        specs.append({"Spec": spec})
        masks.append(ready_mask if pool is None else pool_mask[pool])
        mine = sorted(members[pool]) if pool is not None else list(range(n_nodes))
        for j in range(rng.choice([0, 3, 20])):   # the service runs already: half of it outside its pool
            i = rng.randrange(n_nodes) if j % 2 else rng.choice(mine)
            ev.append(("create_task", running("run%d_%d" % (s, j), "svc%d" % s, "n%05d" % i)))
    facts, tid, left = [], 0, 400
    for tick in range(2):
        rows, prefs = [], []
        for _ in range(rng.randrange(2, 7)):
            s = rng.randrange(n_spread)
            for _ in range(min(left, rng.choice([1, 5, 10, 30]))):
                ev.append(("create_task", dict(sc.pending("t%05d" % tid, "svc%d" % s), **specs[s])))
                rows.append(masks[s])
                prefs.append(1)
                tid += 1
                left -= 1
            for _ in range(min(left, rng.choice([1, 2, 3, 8, 20, 63, 64, 80]))):
                s = n_spread + rng.randrange(n_plain)
                ev.append(("create_task", dict(sc.pending("t%05d" % tid, "svc%d" % s), **specs[s])))
                rows.append(masks[s])
                prefs.append(0)
                tid += 1
                left -= 1
        ev.append(("tick",))
        facts.append(cut_facts(rows, prefs))
    return ev, facts


FIRST, SEEDS = int(os.environ.get("SWP_FUZZ_FIRST", "0")), int(os.environ.get("SWP_FUZZ_SEEDS", "32"))


@pytest.mark.parametrize("seed", range(FIRST, FIRST + SEEDS))
def test_fuzz(seed):
    ev, _ = fuzz_script(seed)
    run_script("cut_fuzz%d" % seed, ev)


def fuzz_coverage(first=FIRST, seeds=SEEDS):
    at_plain = at_pref = own = 0
    for seed in range(first, first + seeds):
        _, facts = fuzz_script(seed)
        at_plain += any(f[1] for f in facts)
        at_pref += any(f[2] for f in facts)
        own += any(f[3] for f in facts)
    return at_plain, at_pref, own


def test_fuzz_seeds_cover_the_ground():
    """Over the seeds, from the scripts alone (the rule restated above on rows built from the labels): at least 8 seeds have a segment
    cut at a plain task, at least 8 one cut at a task with preferences, and none is refused for an own row."""
    at_plain, at_pref, own = fuzz_coverage()
    assert own == 0
    if SEEDS >= 32:
        assert at_plain >= 8 and at_pref >= 8, (at_plain, at_pref)


# ------------------------------------------------------------------------------------------------------------------ the host layer
def host_script():
    """A task group (a SpecVersion) constrained to the pool and the riders' one-off tasks, on 4 200 nodes."""
    ev = pool_nodes(mem_gib=lambda i: 1 + i % 3) + [("set_service", s) for s in ("a", "b", "c", "g")]
    for i in range(40):
        ev.append(("create_task", sc.pending("g%03d" % i, "g", 1, Spec={"Placement": {"Constraints": ["node.labels.pool==a"]}})))
    tasks, runs, gaps, with_prefs = riders_tasks(runs=30)
    return ev + tasks + [("tick",), ("tick",)], runs, gaps, with_prefs


def test_host_layer_keeps_the_tick_one_batch(monkeypatch):
    monkeypatch.setenv("SWP_HOST", "cxx")
    monkeypatch.setenv("SWP_SCHED_ONEOFF_SPREAD", "1")
    ev, runs, gaps, with_prefs = host_script()
    want_ticks, want_rows = oracle_of("cut_host", ev)
    s, k = swhost.HostScheduler(), 0
    for x in ev:
        if x[0] == "tick":
            b0 = s.e.stats()["batches"]
            got = sorted(key(d) for d in s.tick())
            assert got == want_ticks[k], (k, [(a, b) for a, b in zip(want_ticks[k], got) if a != b][:5])
            if k == 0:
                st = s.e.stats()   # the call for the task group, then ONE batch: a spread segment per run, rounds for the riders
                assert st["batches"] == b0 + 2, st
                assert st["scan_launches"] >= runs and st["scan_tasks"] >= with_prefs and st["resolve_launches"] > 0, st
            k += 1
        else:
            getattr(s, x[0])(*x[1:])
    for nid, a in want_rows.items():
        b = s.node_info(nid)
        assert a["ActiveTasksCount"] == b["ActiveTasksCount"] and a["AvailableResources"]["MemoryBytes"] == b["AvailableResources"]["MemoryBytes"], nid


def test_without_the_knob_the_host_layer_splits_as_before(monkeypatch):
    monkeypatch.setenv("SWP_HOST", "cxx")
    ev, runs, gaps, with_prefs = host_script()
    want_ticks, _ = oracle_of("cut_host", ev)
    s = swhost.HostScheduler()
    for x in ev[:-1]:
        if x[0] == "tick":
            assert sorted(key(d) for d in s.tick()) == want_ticks[0]
            # (the task group in one call; a call for a group of one per task with preferences; a batch per gap of riders)
            assert s.e.stats()["batches"] == 1 + with_prefs + gaps
        else:
            getattr(s, x[0])(*x[1:])
