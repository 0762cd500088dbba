"""CPU: preassigned tasks with cluster mounts inside the batched walk. The header declares swp_fit_pairs_volumes, libswp.so exports it
and its device code passes tools/check_kernels.py; and processPreassignedTasks of the C++ host layer (swarmkit_amd/csrc/swp_sched.cpp)
over an engine double WITH that entry (tests/fakefitvol.py: mount tasks join the run, one engine call per run) answers every question
exactly as over the plain double (no pair entry: one swp_check_node + swp_choose_volumes + swp_commit per task). The double's verdicts
and volume choices are pseudo-random in call order, so equal answers mean the batched path judged the same tasks in the same order,
chose for the same tasks and booked what the per-task path books — decisions, node infos, the volumes' users and per-node counts
(bookChooseRemainder: a volume picked for m mounts of a task leaves m - 1 counts), freeVolumes."""
import os
import random
import re
import subprocess
import sys

import pytest

import fakefitvol
import fakelib
import orc
from swarmkit_amd import abi, sched as swsched

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_the_entry_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "swp.h")).read()
    assert re.search(r"^int swp_fit_pairs_volumes\(", header, re.M) and "#define SWP_FIT_NO_VOLUME 8" in header
    assert "swp_fit_pairs_volumes" in abi.EXPORTS
    L = abi.load_library(abi.build_library())
    assert hasattr(L, "swp_fit_pairs_volumes")
    assert abi.FIT_NO_VOLUME == 8 and hasattr(abi.Engine, "fit_pairs_volumes")


def test_the_mount_pair_kernel_ships_and_passes_the_kernel_checks():
    abi.build_library()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_kernels.py"), "--verbose"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    line = [l for l in r.stdout.splitlines() if " k_fit_pairs_vol " in l]
    assert len(line) == 1, r.stdout
    assert " scratch    0 " in line[0] and "vgpr-spill 0" in line[0], line[0]


class Twin:
    """The same events into a host layer over each library; every answer compared."""

    def __init__(self):
        self.plain = swsched.Scheduler(engine=abi.Engine(lib_path=fakelib.build()))
        self.lib = fakefitvol.build()
        self.vol = swsched.Scheduler(engine=abi.Engine(lib_path=self.lib))
        self.steps = 0
        self.vols = []

    def both(self, name, *args):
        self.steps += 1
        res = []
        for s in (self.plain, self.vol):
            try:
                res.append(("ok", getattr(s, name)(*args)))
            except abi.Unsupported:
                res.append(("unsupported", None))
        assert res[0] == res[1], (self.steps, name, args[:1], res)
        return res[0][1]

    def calls(self):
        return fakefitvol.calls(self.lib)

    def books(self, node_ids):
        for n in node_ids:
            self.both("node_info", n)
        for v in self.vols:
            self.both("volume_info", v)
        self.both("free_volumes")


def _node(i):
    return {"ID": "n%03d" % i, "Status": {"State": 2}, "Spec": {"Availability": 0},
            "Description": {"Hostname": "h%d" % i, "Resources": {"NanoCPUs": 8 * 10**9, "MemoryBytes": 16 << 30}, "CSIInfo": [{"PluginName": "csi-a", "NodeID": "c%d" % i}]}}


def _volume(p, vid, group, scope="MULTI_NODE", sharing="ALL", availability="ACTIVE", published=()):
    p.both("update_volume", {"ID": vid, "Spec": {"Annotations": {"Name": "name-" + vid}, "Group": group, "Driver": {"Name": "csi-a"},
                                                 "AccessMode": {"Scope": scope, "Sharing": sharing}, "Availability": availability},
                             "VolumeInfo": {"VolumeID": "plug-" + vid, "AccessibleTopology": []},
                             "PublishStatus": [{"NodeID": n, "State": "PUBLISHED"} for n in published]})
    p.vols.append(vid)


def _mount(source, target="/data", ro=False):
    return {"Type": 4, "Source": source, "Target": target, "ReadOnly": ro}


def _task(tid, sid, node, mounts=None, **kw):
    t = {"ID": tid, "ServiceID": sid, "DesiredState": orc.RUNNING, "Status": {"State": orc.PENDING}, "NodeID": node,
         "Spec": {"Resources": {"Reservations": {"NanoCPUs": 10**8, "MemoryBytes": 64 << 20}}}}
    if mounts is not None:
        t["Spec"]["Container"] = {"Mounts": mounts}
    t.update(kw)
    return t


# what the global services of the scripts below mount (None: nothing)
SHAPES = {
    "one-group": [_mount("group:g")],
    "same-volume-twice": [_mount("group:solo", "/a"), _mount("group:solo", "/b")],          # one volume for two mounts: the m - 1 count
    "second-mount-finds-none": [_mount("group:g", "/a"), _mount("group:nobody", "/b")],     # chooseTaskVolumes fails at the second mount
    "read-only-on-one-writer": [_mount("group:w", "/w", ro=True)],                          # ONE_WRITER with a writer: a reader still fits
    "paused-volume": [_mount("name-vpaused")],                                              # Availability != ACTIVE
    "named-and-group": [_mount("name-v0", "/n"), _mount("group:g", "/g", ro=True), _mount("group:solo", "/s")],
    "plain": None,
}


def _cluster(p, n_nodes):
    nodes = [_node(i) for i in range(n_nodes)]
    for d in nodes:
        p.both("create_node", d)
    ids = [d["ID"] for d in nodes]
    _volume(p, "v0", "g", published=ids[::2])
    _volume(p, "v1", "g", scope="SINGLE_NODE", sharing="ALL")
    _volume(p, "vsolo", "solo", published=ids[:2])
    _volume(p, "vw", "w", sharing="ONE_WRITER")
    _volume(p, "vpaused", "p", availability="PAUSE")
    # a writer on the ONE_WRITER volume, found on its node at start-up (setupTasksList reserves its volumes)
    p.both("set_service", "writer")
    p.both("setup_task", _task("w0", "writer", ids[0], [_mount("group:w", "/w")], Status={"State": orc.RUNNING},
                               Volumes=[{"ID": "vw", "Source": "group:w", "Target": "/w"}]))
    return ids


@pytest.mark.parametrize("seed", range(10))
def test_mount_tasks_join_the_run_and_decide_as_the_per_task_path(seed):
    rng = random.Random(0x7017 + seed)
    p = Twin()
    ids = _cluster(p, rng.choice([2, 5, 16, 33]))
    shapes = sorted(SHAPES)
    services = {}
    for k in range(rng.randrange(3, 8)):
        sid = ("fits-%d" if rng.random() < 0.5 else "svc-%d") % k      # ("fits...": the double's check always passes)
        services[sid] = shapes[k % len(shapes)] if k < len(shapes) else rng.choice(shapes)
        p.both("set_service", sid)
    tid = 0
    for rnd in range(3):
        # one pending task per node and service, services and nodes interleaved
        order = [(n, sid) for n in ids for sid in sorted(services)]
        rng.shuffle(order)
        for n, sid in order:
            if rng.random() < 0.15:
                continue
            kw = {}
            if rng.random() < 0.1:
                kw["DesiredState"] = orc.SHUTDOWN
            p.both("create_task", _task("t%05d" % tid, sid, n if rng.random() > 0.03 else "n-unknown", SHAPES[services[sid]], **kw))
            tid += 1
        f0, v0 = p.calls()
        d = p.both("process_preassigned")
        f1, v1 = p.calls()
        assert (f1 - f0) + (v1 - v0) <= 1                                 # nothing here ends a run: one engine call for the whole pending list
        placed = [x for x in d if x["State"] >= orc.ASSIGNED]
        p.books(ids[:6])
        for x in rng.sample(placed, min(len(placed), 4)):                 # tasks going away: room and volumes free again
            p.both("delete_task", {"ID": x["ID"], "ServiceID": x["ServiceID"], "NodeID": x["NodeID"], "Status": {"State": orc.RUNNING}, "Volumes": x.get("Volumes") or []})
        p.both("process_preassigned")
        p.both("tick")
        p.books(ids[:6])


def test_one_engine_call_for_a_run_that_mixes_mount_and_plain_tasks():
    """The parent needed one call per run BETWEEN mount tasks plus the per-task calls of every mount task; now the pending list is one run."""
    p = Twin()
    ids = _cluster(p, 4)
    for sid, shape in (("fits-a", "plain"), ("fits-m1", "one-group"), ("fits-b", "plain"), ("fits-m2", "same-volume-twice"),
                       ("fits-m3", "second-mount-finds-none"), ("fits-ro", "read-only-on-one-writer"), ("fits-p", "paused-volume")):
        p.both("set_service", sid)
        for k, n in enumerate(ids):
            p.both("create_task", _task("%s-%d" % (sid, k), sid, n, SHAPES[shape]))
    f0, v0 = p.calls()
    d = p.both("process_preassigned")
    f1, v1 = p.calls()
    assert (f1 - f0, v1 - v0) == (0, 1)
    by = {x["ID"]: x for x in d}
    assert len(by) == 7 * len(ids)
    assert all(by["fits-a-%d" % k]["State"] == orc.ASSIGNED for k in range(len(ids)))
    # a failed choice: every filter passed, the task keeps its state with the reference's error and is not on its node
    lost = [x for x in d if x["Err"].startswith("cannot find volume to satisfy mount with source ")]
    assert lost and all(x["State"] == orc.PENDING and not x.get("Volumes") for x in lost)
    assert all(by["fits-m3-%d" % k] in lost for k in range(len(ids)))
    # attachments in mount order, one per mount; the doubled volume leaves its count behind (compared in books())
    twice = [by["fits-m2-%d" % k] for k in range(len(ids)) if by["fits-m2-%d" % k]["State"] == orc.ASSIGNED]
    assert twice and all([v["ID"] for v in x["Volumes"]] == ["vsolo", "vsolo"] and [v["Target"] for v in x["Volumes"]] == ["/a", "/b"] for x in twice)
    p.books(ids)
    counted = p.vol.volume_info("vsolo")["Nodes"]
    assert sum(counted.values()) >= len(twice)
    # a run without any mount template keeps the plain entry
    q = Twin()
    ids = _cluster(q, 3)
    q.both("set_service", "fits-c")
    for k, n in enumerate(ids):
        q.both("create_task", _task("c-%d" % k, "fits-c", n))
    f0, v0 = q.calls()
    q.both("process_preassigned")
    f1, v1 = q.calls()
    assert (f1 - f0, v1 - v0) == (1, 0)


def test_a_refused_call_with_mounts_takes_the_per_task_path():
    p = Twin()
    ids = _cluster(p, 2)
    for sid in ("fits-m", "boom-pre", "ok"):
        p.both("set_service", sid)
    p.both("create_task", _task("m1", "fits-m", ids[0], SHAPES["one-group"]))
    p.both("create_task", _task("pb", "boom-pre", ids[0], SHAPES["one-group"]))
    p.both("create_task", _task("p2", "ok", ids[1]))
    p.both("create_task", _task("m2", "fits-m", ids[1], SHAPES["same-volume-twice"]))
    f0, v0 = p.calls()
    d = p.both("process_preassigned")
    by = {x["ID"]: x for x in d}
    assert by["pb"].get("Deferred") is True and "refused" in by["pb"]["Err"]
    assert not any(by[t].get("Deferred") for t in ("m1", "p2", "m2"))
    assert p.calls() == (f0, v0 + 1)
    p.books(ids)


def _runtime(name):
    q = subprocess.run(["gcc", "-print-file-name=" + name], capture_output=True, text=True).stdout.strip()
    return q if os.path.isabs(q) and os.path.exists(q) else None


def test_this_file_under_the_sanitizers():
    if os.environ.get("SWP_FAKE_SANITIZE") == "1":
        return   # (the child run)
    asan, ubsan = _runtime("libasan.so"), _runtime("libubsan.so")
    if not asan or not ubsan:
        pytest.skip("no sanitizer runtimes next to this gcc")
    env = dict(os.environ, SWP_FAKE_SANITIZE="1", LD_PRELOAD=asan + ":" + ubsan, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "run or refused"],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
