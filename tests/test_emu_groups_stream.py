"""CPU: the STREAMED instance of the task-group kernel (swarmkit_amd/csrc/swp_groups.hpp k_groups2s: the machine's G2_OP_PUBLISH
command behind a group, helper 0's copy / fence / mark / counter, the cancel word) run on fibers against the sequential model of
tests/emu/emu_groups.cpp (tests/emu/emu_groups_stream.cpp includes that file: the same problems, the same model). At every release
store of the mark counter the program stands where the polling host stands: the placements in front of the mark are the model's final
ones, no sentinel among them. At the end: the marks are the host rule's (swp_rounds.hpp group_marks), every output and all mutated
state are the model's, and the 16-entry command ring never held more than 16 commands a helper had not read (asserted at every post).
Built twice: with the product's LDS arena and with a tiny one (the global-memory instance of the machine). No GPU involved; the GPU
parity is tests/test_engine_groups_stream.py. emu_groups.cpp and wv_emu.hpp are not touched: the new primitives' CPU twins are in
tests/emu/wv_emu_sys.hpp."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
CSRC = os.path.join(HERE, "..", "swarmkit_amd", "csrc")


def build(name, flags):
    out = os.path.join(HERE, "_build", name)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    srcs = [os.path.join(EMU, f) for f in ("emu_groups_stream.cpp", "emu_groups.cpp", "wv_emu.hpp", "wv_emu_sys.hpp")] + \
        [os.path.join(CSRC, f) for f in ("swp_groups.hpp", "swp_types.hpp", "swp_rounds.hpp", "swp_volumes.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs):
        tmp = out + ".%d.tmp" % os.getpid()   # (xdist workers may build at the same time)
        subprocess.run(["g++", "-O1", "-std=c++17"] + flags + ["-o", tmp, srcs[0]], check=True)
        os.replace(tmp, out)
    return out


@pytest.fixture(scope="module")
def emu_lds():
    return build("emu_groups_stream", [])


@pytest.fixture(scope="module")
def emu_global():
    return build("emu_groups_stream_small", ["-DG2_ARENA_LDS=3072"])


def run(binary, case, step, cancel_at=0, sched=None, extra=()):
    env = dict(os.environ)
    env.pop("EMU_SCHED_SEED", None)
    if sched:
        env["EMU_SCHED_SEED"] = str(sched)
    r = subprocess.run([binary] + [str(x) for x in case] + [str(step), str(cancel_at), "v"] + list(extra), capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "-> OK" in r.stderr, r.stderr[-2000:]
    return r.stderr


# (seed, nodes, groups, largest group, spread trees, feature level, threads) as tests/test_emu_groups.py; feature 3: host ports, uncounted
# tasks and generic reservations (the unfused write-back), and one group in seven of the service before it (nothing evaluated ahead)
CASES = [
    (32, 70, 40, 30, 3, 3, 256),       # 40 groups, step 1: about 170 commands through the ring of 16
    (14, 500, 16, 80, 4, 3, 1024),     # the product's geometry: 15 helper waves
    (41, 1500, 30, 5, 4, 3, 256),      # groups of a handful of tasks
    (3, 300, 12, 60, 1, 0, 128),       # a single helper wave: it publishes and does everything else
    (23, 400, 14, 900, 5, 3, 256),     # groups far larger than the node set: -1 in the stream
]
IDS = lambda c: "seed%d-N%d-g%d-k%d-t%d-f%d-w%d" % (c[0], c[1], c[2], c[3], c[4], c[5], c[6] // 64)   # noqa: E731


@pytest.mark.parametrize("step", [1, 64, 100000])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_published_prefixes_are_final_and_the_marks_are_the_hosts(emu_lds, case, step):
    err = run(emu_lds, case, step)
    m = re.search(r"same service as the one before: (\d+), ports or generic: (\d+)\) (\d+) tasks, step (\d+): (\d+) marks, (\d+) commands posted, ring occupancy at most (\d+) of 16", err)
    assert m, err[-500:]
    deps, special, total, got_step, marks, posted, occ = (int(x) for x in m.groups())
    assert got_step == step and total > 0 and occ <= 16   # (fewer than 2048 groups: the ring bound leaves the knob alone)
    if got_step == 1:
        assert marks == case[2]
    if step == 100000:
        assert marks == 1
    if case[0] == 32:
        assert deps >= 1 and special >= 5            # the shapes the case is there for
        if step == 1:
            assert posted > 5 * 16                   # the ring wrapped many times


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[4]], ids=IDS)
def test_global_memory_instance(emu_global, case):
    run(emu_global, case, 1)


@pytest.mark.parametrize("sched", [51, 7])
@pytest.mark.parametrize("arena", ["lds", "global"])
@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[3]], ids=IDS)
def test_under_random_wave_schedules(emu_lds, emu_global, case, arena, sched):
    """The publishing helper far behind the machine, far ahead of the other helpers, one wave at a time (EMU_SCHED_SEED, wv_emu.hpp)."""
    run(emu_lds if arena == "lds" else emu_global, case, 1, sched=sched)


@pytest.mark.parametrize("sched", [None, 51, 9])
@pytest.mark.parametrize("case,cancel_at", [(CASES[0], 3), (CASES[0], 40), (CASES[1], 1), (CASES[2], 11)], ids=lambda v: IDS(v) if isinstance(v, tuple) else "mark%d" % v)
def test_a_cancel_word_ends_the_launch(emu_lds, case, cancel_at, sched):
    """The word is set while the helper stores mark number `cancel_at`: ERR_GROUP_CANCELLED, no hang (the fibers would deadlock and the
    harness abort), the marks seen are a prefix of the host's and lie within the groups the machine went through."""
    err = run(emu_lds, case, 1, cancel_at=cancel_at, sched=sched)
    m = re.search(r"cancelled at mark (\d+) of (\d+), (\d+) marks seen, stopped after group (\d+)", err)
    assert m, err[-500:]
    at, n_marks, seen, stop = (int(x) for x in m.groups())
    assert at == cancel_at and seen >= at and stop <= case[2]
    if cancel_at < n_marks - 8:
        assert stop < case[2]                        # it did not run to the end: at most the commands in flight were still executed


def test_plain_program_still_builds_beside_it():
    """tests/emu/emu_groups.cpp does not define the macro the streamed code sits behind and does not include the new twins: it builds
    from the same header as before."""
    out = os.path.join(HERE, "_build", "emu_groups_beside_stream")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    tmp = out + ".%d.tmp" % os.getpid()
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", tmp, os.path.join(EMU, "emu_groups.cpp")], check=True)
    os.replace(tmp, out)
    src = open(os.path.join(EMU, "emu_groups.cpp")).read()
    assert "SWP_G2_STREAM" not in src and "wv_emu_sys" not in src
