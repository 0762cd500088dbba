"""CPU: the WIDE spread instance of the scan resolver (swarmkit_amd/csrc/swp_scan_spread.hpp k_scan_spread_wide: one-off tasks with
spread preferences and no constraint on a nodeSet of more than 4 096 nodes, decided over ALL node slots with the node rows in global
memory) on fibers against the sequential model of tests/emu/emu_scan_spread_wide.cpp — every output and every mutated array, a guard
zone behind every array the kernel writes; alone, and between two stretches of the block resolver.
No GPU involved; the GPU parity against the oracle is tests/test_engine_oneoff_spread_wide.py."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
BIN = os.path.join(HERE, "_build", "emu_scan_spread_wide")
CSRC = os.path.join(HERE, "..", "swarmkit_amd", "csrc")


@pytest.fixture(scope="module")
def emu_bin():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    srcs = [os.path.join(EMU, "emu_scan_spread_wide.cpp"), os.path.join(EMU, "wv_emu.hpp"), os.path.join(EMU, "emu_model.hpp"),
            os.path.join(CSRC, "swp_scan_spread.hpp"), os.path.join(CSRC, "swp_scan.hpp"), os.path.join(CSRC, "swp_resolve6.hpp"),
            os.path.join(CSRC, "swp_shard.hpp"), os.path.join(CSRC, "swp_types.hpp")]
    if not os.path.exists(BIN) or any(os.path.getmtime(s) > os.path.getmtime(BIN) for s in srcs):
        tmp = BIN + ".%d.tmp" % os.getpid()   # (xdist workers may build at the same time)
        subprocess.run(["g++", "-O1", "-std=c++17", "-o", tmp, srcs[0]], check=True)
        os.replace(tmp, BIN)
    return BIN


# (seed, nodes, tasks, services, block, task order, feature level, spread levels, values per label key, flags)
# feature levels as in test_emu_scan_spread.py: 1 heavy services (tasks that find no node), MaxReplicas, services that already run on
# nodes, >= 5 recent failures; 2 host ports, RT_UNCOUNTED; 3 generic reservations. Flags: see emu_scan_spread_wide.cpp.
CASES = [
    (1, 1024, 150, 4, 64, 0, 1, 2, 3, ""),        # one node a thread
    (2, 1025, 150, 4, 64, 2, 2, 2, 3, "l"),       # two (one thread only); a missing label: the "" branch
    (3, 2049, 200, 6, 64, 0, 3, 3, 3, ""),        # three; generic reservations, three levels
    (4, 4097, 200, 6, 64, 0, 1, 1, 4, "d"),       # beyond the plain limit; a branch found without room
    (5, 9000, 300, 8, 64, 2, 2, 2, 5, "ld"),
    (6, 65536, 20, 3, 64, 0, 0, 1, 3, "h"),       # every slot the key has: the top node bit set on every pick
    (7, 4400, 150, 4, 64, 1, 0, 0, 1, ""),        # no levels at all: every tree is one leaf
    (8, 5000, 200, 4, 64, 0, 1, 2, 4, "a"),       # every node of a thread in one leaf: one fold a task
    (9, 5000, 200, 4, 64, 0, 1, 2, 4, "z"),       # a thread's nodes in alternating leaves: an atomic a node
    (10, 4097, 4, 1, 64, 0, 0, 1, 3, "e"),        # equal keys 1 024 apart (one thread: the fold)
    (11, 65536, 4, 1, 64, 0, 0, 1, 3, "E"),       # equal keys 65 535 apart (two threads: the LDS minimum)
    (12, 4500, 150, 4, 64, 0, 1, 1, 3, "t"),      # nodes that hold 65 535 tasks: legal
    (13, 4500, 60, 4, 64, 0, 0, 1, 3, "T"),       # a node that holds 65 536: ERR_LEVEL_RANGE in front of the first task that could take it
    (14, 4400, 300, 6, 64, 0, 1, 2, 4, "m"),      # between two stretches of the block resolver
    (15, 6000, 300, 6, 64, 2, 3, 3, 3, "l"),
]


def _ids(c):
    return "seed%d-N%d-T%d-f%d-L%d%s" % (c[0], c[1], c[2], c[6], c[7], c[9])


def _run(emu_bin, case, env=None):
    args = [str(x) for x in case[:9]] + ["v"] + list(case[9])
    r = subprocess.run([emu_bin] + args, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "-> OK" in r.stderr
    return r.stderr


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_wide_spread_kernel_source_matches_sequential_model(emu_bin, case):
    out = _run(emu_bin, case)
    m = re.search(r"picks with the top node bit (\d+) \| largest task total of a node (\d+) \| stopped at task (\d+) of (\d+) with error (\d+) \| guard zones checked (\d+)", out)
    top, max_total, stopped, T, error, guards = (int(x) for x in m.groups())
    assert guards == 18   # the sixteen arrays of the state and the two matrices
    m = re.search(r"spread tasks placed (\d+), left without a node (\d+) \| branches found without room (\d+)", out)
    placed, unplaced, noroom = (int(x) for x in m.groups())
    flags = case[9]
    if case[7] and "T" not in flags:
        assert placed > 0, out[-500:]
    if "h" in flags:
        assert top > 0 and top == int(re.search(r": placed (\d+) inf", out).group(1)), out[-500:]   # (tasks without preferences included)
    if "d" in flags:
        assert noroom > 0, out[-500:]
    if "t" in flags:
        assert max_total == 65535 and error == 0, out[-500:]
    if "T" in flags:
        assert error == 1 and 0 < stopped < T, out[-500:]   # ERR_LEVEL_RANGE (swp_types.hpp)
    else:
        assert error == 0 and stopped == T, out[-500:]
    if "m" in flags:
        assert int(re.search(r"launches (\d+)", out).group(1)) >= 3, out[-500:]


@pytest.mark.parametrize("sched", [31, 77])
@pytest.mark.parametrize("case", [CASES[4], CASES[8], CASES[13]], ids=_ids)
def test_under_random_wave_schedules(emu_bin, case, sched):
    """... under wave orders the first-in-first-out run never produces (EMU_SCHED_SEED, tests/emu/wv_emu.hpp)."""
    _run(emu_bin, case, env=dict(os.environ, EMU_SCHED_SEED=str(sched)))
