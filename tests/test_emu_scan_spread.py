"""CPU: the spread instance of the scan resolver (swarmkit_amd/csrc/swp_scan_spread.hpp: one-off tasks with spread preferences inside a
batch) on fibers against the sequential model of tests/emu/emu_scan_spread.cpp — nodeSet.tree with a heap of one, the literal
scheduleNTasksOnSubtree, NodeInfo.addTask: every output and every mutated array; alone, and between two stretches of the block resolver.
No GPU involved; the GPU parity against the oracle is tests/test_engine_oneoff_spread.py."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
BIN = os.path.join(HERE, "_build", "emu_scan_spread")
CSRC = os.path.join(HERE, "..", "swarmkit_amd", "csrc")


@pytest.fixture(scope="module")
def emu_bin():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    srcs = [os.path.join(EMU, "emu_scan_spread.cpp"), os.path.join(EMU, "wv_emu.hpp"), os.path.join(EMU, "emu_model.hpp"),
            os.path.join(CSRC, "swp_scan_spread.hpp"), os.path.join(CSRC, "swp_scan.hpp"), os.path.join(CSRC, "swp_resolve6.hpp"),
            os.path.join(CSRC, "swp_shard.hpp"), os.path.join(CSRC, "swp_types.hpp")]
    if not os.path.exists(BIN) or any(os.path.getmtime(s) > os.path.getmtime(BIN) for s in srcs):
        tmp = BIN + ".%d.tmp" % os.getpid()   # (xdist workers may build at the same time)
        subprocess.run(["g++", "-O1", "-std=c++17", "-o", tmp, srcs[0]], check=True)
        os.replace(tmp, BIN)
    return BIN


# (seed, nodes, tasks, services, block, task order, feature level, spread levels, values per label key, flags)
# feature levels as in test_emu_scan.py: 1 heavy services (tasks that find no node), MaxReplicas, services that already run on nodes,
# >= 5 recent failures; 2 host ports, RT_UNCOUNTED; 3 generic reservations. Flags: see emu_scan_spread.cpp.
CASES = [
    (1, 3, 1, 1, 64, 0, 0, 2, 2, "x"),          # the two-level X / Y shape: the branch that is handed five tasks picks rack A
    (1, 1, 5, 1, 64, 0, 0, 1, 2, ""),           # one node
    (2, 63, 200, 4, 64, 0, 1, 1, 3, ""),
    (2, 64, 200, 4, 64, 0, 1, 2, 3, ""),
    (2, 65, 200, 4, 64, 2, 2, 2, 3, "l"),       # ... a missing label: the "" branch
    (3, 300, 800, 10, 64, 0, 2, 2, 3, "l"),
    (4, 300, 800, 10, 64, 2, 3, 3, 4, "d"),     # three levels; a first-level branch whose nodes fail every class and carry tasks
    (6, 200, 500, 6, 64, 1, 1, 1, 1, ""),       # one level of ONE value: a root with one child
    (7, 200, 500, 6, 64, 0, 1, 0, 1, ""),       # no levels at all: every tree is one leaf (k_scan's answers)
    (8, 150, 400, 5, 64, 0, 1, 1, 6, "d"),      # one level, one branch without room
    (9, 1024, 500, 8, 64, 0, 2, 2, 5, ""),
    (5, 1025, 600, 8, 64, 0, 1, 2, 5, "m"),     # two nodes a thread; the block resolver in front of and behind the segment
    (10, 300, 900, 12, 64, 2, 3, 3, 3, "ml"),
    (11, 4096, 300, 6, 256, 0, 1, 2, 6, "m"),   # the most nodes the kernel takes (four per thread)
    (12, 40, 600, 3, 32, 0, 1, 3, 2, "d"),      # few nodes, many tasks: most find no node
]
NOROOM = {4, 8, 12}   # cases that must have met a branch without room


def _ids(c):
    return "seed%d-N%d-T%d-f%d-L%d%s" % (c[0], c[1], c[2], c[6], c[7], c[9])


def _run(emu_bin, case, env=None):
    args = [str(x) for x in case[:9]] + ["v"] + list(case[9])
    r = subprocess.run([emu_bin] + args, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "-> OK" in r.stderr
    return r.stderr


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_spread_kernel_source_matches_sequential_model(emu_bin, case):
    out = _run(emu_bin, case)
    m = re.search(r"spread tasks placed (\d+), left without a node (\d+) \| branches found without room (\d+) \| calls that handed a branch more than one task (\d+)", out)
    placed, unplaced, noroom, more = (int(x) for x in m.groups())
    if case[7]:
        assert placed > 0, out[-500:]
    if case[0] in NOROOM:
        assert noroom > 0 and unplaced > 0, out[-500:]
    if "x" in case[9]:
        assert more > 0, out[-500:]


@pytest.mark.parametrize("sched", [31, 77])
@pytest.mark.parametrize("case", [CASES[4], CASES[6], CASES[11], CASES[12], CASES[13]], ids=_ids)
def test_under_random_wave_schedules(emu_bin, case, sched):
    """... under wave orders the first-in-first-out run never produces (EMU_SCHED_SEED, tests/emu/wv_emu.hpp)."""
    _run(emu_bin, case, env=dict(os.environ, EMU_SCHED_SEED=str(sched)))
