"""CPU: assigned generic resources in the enforcer sweep. The header declares swp_enforce_generic, libswp.so exports it, the binding has
it and its kernel passes tools/check_kernels.py; and `enforce` of the C++ host layer (swarmkit_amd/csrc/swp_sched.cpp) over an engine
double WITH that entry (tests/fakeenforce.py: one engine call for the whole request, the lists travelling as kind / name ids) answers
exactly as over the plain double (swp_enforce, then the host layer's own walk over std::string lists).

The double scripts the verdicts of the loop's first two thirds (constraints, cpu / mem): pseudo-random per task, in call order, so they
say nothing about the request's constraints. The oracle is still the judge of the generic third: the scripted verdicts are read from
the double's call log and handed to orc.enforce as facts — a task the double rejected gets a constraint no node meets, a task it kept
loses its constraints and reservations — so that the oracle walks the same kept tasks over the same lists (_as_the_double_saw_it)."""
import os
import random
import re
import subprocess
import sys

import pytest

import fakeenforce
import fakelib
import orc
from swarmkit_amd import abi, sched as swsched

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_the_entry_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "swp.h")).read()
    assert re.search(r"^int swp_enforce_generic\(", header, re.M) and "} swp_enforce_res;" in header
    assert "swp_enforce_generic" in abi.EXPORTS and "swp_enforce_generic" in abi.OPTIONAL
    L = abi.load_library(abi.build_library())
    assert hasattr(L, "swp_enforce_generic")
    assert abi.ENF_RES_DTYPE.itemsize == 16 and hasattr(abi.Engine, "enforce_generic")
    assert not hasattr(abi.load_library(fakelib.build()), "swp_enforce_generic")   # the plain double keeps the host layer's own walk alive


def test_the_kernel_ships_and_passes_the_kernel_checks():
    abi.build_library()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_kernels.py"), "--verbose"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    line = [l for l in r.stdout.splitlines() if " k_enforce_generic " in l]
    assert len(line) == 1, r.stdout
    assert " scratch    0 " in line[0] and "vgpr-spill 0" in line[0], line[0]


KINDS = ["gpu", "fpga", "tpu"]


def _entry(rng, kind=None, long_names=False):
    kind = kind or rng.choice(KINDS)
    if rng.random() < 0.5:
        return {"Named": {"Kind": kind, "Value": "%s%d" % (kind[0], rng.randrange(90 if long_names else 5))}}
    return {"Discrete": {"Kind": kind, "Value": rng.choice([0, 2**30 + 7, -1]) if rng.random() < 0.2 else rng.randrange(1, 5)}}


def _request(seed, with_assignments=True):
    """Nodes whose lists one count per kind cannot stand for (a kind twice, Discrete and Named under one kind, a list of 70+), tasks in
    every state with none, an empty, one, or several assignments (two of one kind among them), some nodes without any generic task."""
    rng = random.Random(0x6E4E + seed)
    nodes, tasks = [], []
    for i in range(rng.choice([1, 4, 9])):
        long_list = rng.random() < 0.25
        lst = [_entry(rng, long_names=long_list) for _ in range(rng.randrange(65, 90) if long_list else rng.randrange(0, 7))]
        nd = {"ID": "n%02d" % i, "Spec": {"Availability": rng.choice([0, 0, 0, 0, 2])}, "Status": {"State": orc.READY},
              "Description": {"Resources": {"NanoCPUs": 4 * 10**9, "MemoryBytes": 8 << 30, "Generic": lst}}}
        if rng.random() < 0.1:
            del nd["Description"]
        nodes.append(nd)
        generic_node = with_assignments and rng.random() < 0.8
        for j in range(rng.randrange(0, 9)):
            t = {"ID": "t%02d-%02d" % (i, rng.randrange(100)), "NodeID": nd["ID"], "ServiceID": "s%d" % rng.randrange(3),
                 "DesiredState": rng.choice([orc.RUNNING] * 5 + [orc.NEW, orc.SHUTDOWN]), "Status": {"State": rng.choice([orc.RUNNING] * 5 + [orc.COMPLETE, orc.FAILED])},
                 "Spec": {"Resources": {"Reservations": {"NanoCPUs": 10**8, "MemoryBytes": 64 << 20}}} if rng.random() < 0.5 else {}}
            if generic_node and rng.random() < 0.6:
                a = []
                for _ in range(rng.randrange(0, 4)):
                    if lst and rng.random() < 0.75:
                        x = rng.choice(lst)
                        x = {k: dict(v) for k, v in x.items()}
                        if "Discrete" in x and 1 < x["Discrete"]["Value"] < 100:
                            x["Discrete"]["Value"] = rng.randrange(1, x["Discrete"]["Value"] + 1)
                    else:
                        x = _entry(rng)
                    if a and rng.random() < 0.3:   # a second assignment of the kind in front of it
                        x = _entry(rng, kind=list(a[-1].values())[0]["Kind"])
                    a.append(x)
                t["AssignedGenericResources"] = a
            tasks.append(t)
    tasks = list({t["ID"]: t for t in tasks}.values())
    tbn = {}
    for t in tasks:
        tbn.setdefault(t["NodeID"], []).append(t)
    services = {"s0": {"ID": "s0", "Spec": {"Task": {"Placement": {"Constraints": ["node.labels.zone==a"]}}}}}
    return nodes, tbn, services


def _scripted_verdicts(engine):
    """The double's swp_enforce verdicts of the last request, in record order (its call log: "  task ... -> 0|1")."""
    return [int(l.rsplit("-> ", 1)[1]) for l in fakelib.take_log(engine) if l.startswith("  task ")]


def _as_the_double_saw_it(nodes, tbn, verdicts):
    """{node id: orc.enforce(...)} with the double's verdicts for the loop's first two thirds taken as facts (module docstring)."""
    out, k = {}, 0
    for nd in nodes:
        if nd["Spec"]["Availability"] != 0:
            continue
        mine = []
        for t in sorted(tbn.get(nd["ID"], []), key=lambda t: t["ID"]):
            v, k = verdicts[k], k + 1
            skipped = not (orc.ASSIGNED <= t["DesiredState"] <= orc.COMPLETE) or t["Status"]["State"] >= orc.COMPLETE
            u = {"ID": t["ID"], "NodeID": t["NodeID"], "DesiredState": t["DesiredState"], "Status": t["Status"], "Spec": {}}
            if v:      # rejected, whatever its states were: `continue` without a claim
                u.update(DesiredState=orc.RUNNING, Status={"State": orc.RUNNING}, Spec={"Placement": {"Constraints": ["node.labels.no-such-label==x"]}})
            elif not skipped and "AssignedGenericResources" in t:
                u["AssignedGenericResources"] = t["AssignedGenericResources"]
            mine.append(u)
        out[nd["ID"]] = orc.enforce(nd, mine, {})
    assert k == len(verdicts)
    return out


def _both(nodes, tbn, services):
    lib = fakeenforce.build()
    plain = swsched.Scheduler(engine=abi.Engine(lib_path=fakelib.build()))
    gen = swsched.Scheduler(engine=abi.Engine(lib_path=lib))
    for s in (plain, gen):
        for nd in nodes:
            s.create_node(nd)
        fakelib.take_log(s.e)
    c0 = fakeenforce.calls(lib)
    got_plain = plain.enforce(nodes, tbn, services)
    got_gen = gen.enforce(nodes, tbn, services)
    return got_plain, got_gen, fakeenforce.calls(lib) - c0, _scripted_verdicts(plain.e), _scripted_verdicts(gen.e)


@pytest.mark.parametrize("seed", range(24))
def test_seeded_requests_one_call_and_the_same_answer(seed):
    nodes, tbn, services = _request(seed)
    got_plain, got_gen, n_calls, v_plain, v_gen = _both(nodes, tbn, services)
    assert got_gen == got_plain
    assert v_gen == v_plain                                     # the double's swp_enforce saw the same records in the same order
    assert got_gen == _as_the_double_saw_it(nodes, tbn, v_gen)
    listed = [t for nd in nodes if nd["Spec"]["Availability"] == 0 for t in tbn.get(nd["ID"], [])]
    assert n_calls == (1 if any(t.get("AssignedGenericResources") for t in listed) else 0)


def test_the_seeds_reach_the_cases():
    """Taken from the requests and the oracle's answers alone: requests with and without assignments, a break with a task behind it,
    a list longer than 64 entries under a task with assignments, a kind twice, mixed types under one kind, two assignments of a kind."""
    seen = dict.fromkeys(["with", "without", "long", "kind_twice", "mixed", "two_of_a_kind", "rejected_generic"], 0)
    for seed in range(24):
        nodes, tbn, _ = _request(seed)
        any_a = False
        for nd in nodes:
            if nd["Spec"]["Availability"] != 0:
                continue
            mine = tbn.get(nd["ID"], [])
            has = [t for t in mine if t.get("AssignedGenericResources")]
            any_a = any_a or bool(has)
            lst = (nd.get("Description") or {}).get("Resources", {}).get("Generic", [])
            if has:
                kinds = [(list(x.values())[0]["Kind"], list(x)[0]) for x in lst]
                seen["long"] += len(lst) > 64
                seen["kind_twice"] += any(kinds.count(k) > 1 for k in kinds if k[1] == "Discrete")
                seen["mixed"] += any((k, "Named") in kinds for k, ty in kinds if ty == "Discrete")
                for t in has:
                    ks = [list(x.values())[0]["Kind"] for x in t["AssignedGenericResources"]]
                    seen["two_of_a_kind"] += len(set(ks)) < len(ks)
                plain = [dict(t, Spec={}) for t in sorted(mine, key=lambda t: t["ID"])]
                bare = [{k: v for k, v in t.items() if k != "AssignedGenericResources"} for t in plain]
                seen["rejected_generic"] += orc.enforce(nd, plain, {}) != orc.enforce(nd, bare, {})
        seen["with" if any_a else "without"] += 1
    assert all(v > 0 for v in seen.values()), seen


def test_a_request_without_assignments_keeps_swp_enforce():
    for seed in range(4):
        nodes, tbn, services = _request(100 + seed, with_assignments=False)
        got_plain, got_gen, n_calls, v_plain, v_gen = _both(nodes, tbn, services)
        assert got_gen == got_plain and v_gen == v_plain and n_calls == 0
    # ... and so does one whose only assignment lists are empty (an empty list behaves like nil)
    nodes, tbn, services = _request(3)
    for lst in tbn.values():
        for t in lst:
            if "AssignedGenericResources" in t:
                t["AssignedGenericResources"] = []
    got_plain, got_gen, n_calls, _, _ = _both(nodes, tbn, services)
    assert got_gen == got_plain and n_calls == 0


def test_the_double_refuses_as_the_engine_does():
    import numpy as np
    e = abi.Engine(lib_path=fakeenforce.build())
    s = swsched.Scheduler(engine=e)
    s.create_node({"ID": "n0", "Spec": {"Availability": 0}, "Status": {"State": orc.READY}})
    kind = e.intern(abi.SPACE_GENERIC_KIND, "gpu")
    nodes = np.zeros(1, dtype=abi.ENF_NODE_DTYPE)
    nodes[0] = (e.intern(abi.SPACE_NODE_ID, "n0"), 0, 2, 0, 0, 0)
    tasks = np.zeros(2, dtype=abi.ENF_TASK_DTYPE)
    tasks["desired_state"] = tasks["state"] = orc.RUNNING
    res = np.array([(kind, 0, 1), (kind, 0, 1)], dtype=abi.ENF_RES_DTYPE)
    for noff, nres, toff, tres in (([0, 1], res[:1], [0, 2, 1], res), ([0, 1], np.array([(kind + 50, 0, 1)], dtype=abi.ENF_RES_DTYPE), [0, 1, 2], res),
                                   ([0, 1], res[:1], [0, 1, 2], np.array([(kind, 2, 1), (kind, 0, 1)], dtype=abi.ENF_RES_DTYPE))):
        out = np.full(2, 7, dtype=np.uint8)
        with pytest.raises(abi.SwpError) as err:
            e.enforce_generic(nodes, tasks, noff, nres, toff, tres, out=out)
        assert err.value.code == abi.SWP_EINVAL and list(out) == [7, 7]


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
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "seeded or without_assignments or refuses"],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
