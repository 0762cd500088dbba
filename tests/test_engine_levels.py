"""GPU: the block resolver's lists over two levels (swp_resolve6.hpp, r6_propose_t "the second section"; the host rule r6_levels2 in
swp_rounds.hpp) against the CPU oracle: 7 000 cfg3 tasks on 2 304 nodes — three laps over the node set, so one class of tasks after
the other finds its level used up inside a block, and 72 half-words, more than a list holds, so the rule's node-set gate is open.
Five runs, each a process of its own under its own time limit, chained so that nothing starts on the device behind a run that
failed: the default; SWP_R6_LEVELS=0; blocks of 1 408 with the drivers' reports on (the count of proposals with a second section);
service-major order (a batch of runs: no long lists, so the switch is off by rule) with and without the knob.
The CPU side, every proposal against the restated rule and every path counted: tests/test_emu_resolve6_levels.py."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "levels_gpu_child.py")
T, BLOCK = 7000, 1408   # (the block the commit kernel's LDS holds for this node set: the reporting run's line says so)


def test_two_level_lists_match_the_oracle_in_fewer_rounds():
    py = sys.executable
    cmd = ("timeout -k 10 120 {py} {c} rr && "
           "timeout -k 10 120 env SWP_R6_LEVELS=0 {py} {c} rr && "
           "timeout -k 10 120 env SWP_R6_BLOCK={b} SWP_DBG=16 {py} {c} rr && "
           "timeout -k 10 120 {py} {c} major && "
           "timeout -k 10 120 env SWP_R6_LEVELS=0 {py} {c} major").format(py=py, c=CHILD, b=BLOCK)
    env = {k: v for k, v in os.environ.items() if k not in ("SWP_R6_BLOCK", "SWP_DBG", "SWP_R6_LEVELS", "SWP_R6_RUNS")}
    r = subprocess.run(["bash", "-c", cmd], capture_output=True, text=True, env=env)
    print(r.stdout[-3000:])
    print(r.stderr[-3000:])
    assert r.returncode == 0, r.stderr[-3000:]   # (every child compared placements and Explain rows with the oracle)
    lines = re.findall(r"^levels-child: order=(\w+) placed=(\d+) unplaceable=(\d+) resolver=(\d+) rounds=(\d+)$", r.stdout, re.M)
    assert [ln[0] for ln in lines] == ["rr", "rr", "rr", "major", "major"], r.stdout
    assert all(int(ln[3]) == 6 for ln in lines), lines          # the block resolver decided every batch
    assert lines[0][1:3] == lines[1][1:3] == lines[2][1:3], lines   # the switch changes the rounds, never the outcome
    rounds = [int(ln[4]) for ln in lines]
    least = (T + BLOCK - 1) // BLOCK
    assert rounds[0] < rounds[1], lines                         # fewer rounds with the second section ...
    assert rounds[0] >= least and rounds[2] >= least, lines     # ... and never fewer than the blocks the batch has
    m = re.search(r"k_resolve6 tasks \[0, %d\): (\d+) rounds of (\d+) .* proposals with a second section (\d+)" % T, r.stderr)
    assert m, r.stderr[-3000:]
    assert int(m.group(2)) == BLOCK and int(m.group(3)) > 0, m.group(0)
    assert rounds[3] == rounds[4], lines                        # a batch of runs: the switch is off by rule, the knob changes nothing
