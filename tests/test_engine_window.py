"""GPU: the block resolver's late-staged list windows (swp_resolve6.hpp, r6_commit_t) against the CPU oracle: 3 000 cfg3 tasks on 4 096
nodes — more than two full blocks, and a level of 4 096 nodes is more than the 32 half-words a proposal itself holds, so the lists
reach into their extension. Three runs, each a process of its own under its own time limit, chained so that nothing starts on the
device behind a run that failed: the default block; blocks of 1 408 tasks with a window of four entries (R6Args.dbg bits 12-16, with
the section timers' report on for its cut counters); service-major order as the engine runs it (a batch of runs: windows of 32 in
blocks of 768, no list extension, staged at once); and service-major order with that policy off (SWP_R6_RUNS=0: the runs-by-rank path
reads a run's list from a 16-entry window of an extended list, in blocks of 1 408).
The CPU side of the same paths, with every case counted: tests/test_emu_resolve6_window.py."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "window_gpu_child.py")
SHORT_WINDOW = (4 << 12) | 16   # SWP_DBG: a window of 4 entries | the drivers' reports


def test_window_staging_matches_the_oracle():
    py = sys.executable
    cmd = ("timeout -k 10 120 {py} {c} rr && "
           "timeout -k 10 120 env SWP_R6_BLOCK=1408 SWP_DBG={dbg} {py} {c} rr && "
           "timeout -k 10 120 {py} {c} major && "
           "timeout -k 10 120 env SWP_R6_RUNS=0 SWP_DBG=16 {py} {c} major").format(py=py, c=CHILD, dbg=SHORT_WINDOW)
    env = {k: v for k, v in os.environ.items() if k not in ("SWP_R6_BLOCK", "SWP_DBG", "SWP_R6_RUNS")}
    r = subprocess.run(["bash", "-c", cmd], capture_output=True, text=True, env=env)
    print(r.stdout[-3000:])
    print(r.stderr[-3000:])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = re.findall(r"^window-child: order=(\w+) placed=(\d+) unplaceable=(\d+) resolver=(\d+) rounds=(\d+)$", r.stdout, re.M)
    assert [ln[0] for ln in lines] == ["rr", "rr", "major", "major"], r.stdout
    assert lines[2][1:3] == lines[3][1:3], lines                # the runs policy changes the rounds, never the outcome
    blocks = re.findall(r"k_resolve6 tasks \[0, 3000\): \d+ rounds of (\d+) ", r.stderr)
    assert blocks == ["1408", "1408"], r.stderr[-3000:]         # (the two runs that report: the short window, the policy off)
    assert all(int(ln[3]) == 6 for ln in lines), lines          # the block resolver decided every batch
    assert lines[0][1:3] == lines[1][1:3], lines                # the window changes the rounds, never the outcome
    # the short-window run: blocks of 1 408, and windows that ran out with entries left were met (and the run still agrees with the oracle)
    m = re.search(r"k_resolve6 tasks \[0, 3000\): (\d+) rounds of (\d+) .* a window that ran out (\d+),", r.stderr)
    assert m, r.stderr[-3000:]
    assert int(m.group(2)) == 1408 and int(m.group(3)) > 0, m.group(0)
    assert int(lines[1][4]) > int(lines[0][4]), lines           # ... which cost rounds
