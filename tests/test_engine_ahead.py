"""GPU: the commit kernel's matcher with the entries at a lane's cursor requested ahead of its stops (swp_resolve6.hpp, r6_commit_t,
R6_SEAT_AHEAD) against the CPU oracle, in the manner of tests/test_engine_heads.py: every run a process of its own under its own time
limit, chained so that nothing starts on the device behind a run that failed — 3 000 cfg3 tasks on 4 096 nodes round-robin in blocks of
1 408, once as in production and once with the section timers' report on, and service-major; 1 200 tasks of 4 services on 96 nodes
(three half-words: the levels run out all the time, many stops a group); and the volume script of tests/bigcases.py at 300 nodes and
900 tasks (k_r6_commit_v). Placements and the explanations of the unplaceable tasks equal the oracle's, and the rounds are the ones the
kernel took before the change (ROUNDS: what tests/heads_gpu_child.py prints for the same shapes, from the commit before this one on
an MI355X; a round's cuts are decided by the lists, not by when a read is issued). The CPU side, with every path counted:
tests/test_emu_resolve6_ahead.py."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "ahead_gpu_child.py")
ROUNDS = {"rr": 3, "major": 5, "dense": 6}


def test_entries_requested_ahead_match_the_oracle():
    py = sys.executable
    cmd = ("timeout -k 10 120 env SWP_R6_BLOCK=1408 {py} {c} rr && "
           "timeout -k 10 120 env SWP_R6_BLOCK=1408 SWP_DBG=16 {py} {c} rr && "
           "timeout -k 10 120 {py} {c} major && "
           "timeout -k 10 120 {py} {c} dense && "
           "timeout -k 10 120 {py} {c} volumes").format(py=py, c=CHILD)
    env = {k: v for k, v in os.environ.items() if k not in ("SWP_R6_BLOCK", "SWP_DBG", "SWP_R6_RUNS", "SWP_R6_TWINS")}
    r = subprocess.run(["bash", "-c", cmd], capture_output=True, text=True, env=env)
    print(r.stdout[-3000:])
    print(r.stderr[-3000:])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = re.findall(r"^ahead-child: what=(\w+) placed=(\d+) unplaceable=(\d+) resolver=(\d+) rounds=(\d+)$", r.stdout, re.M)
    assert [ln[0] for ln in lines] == ["rr", "rr", "major", "dense"], r.stdout
    assert lines[0][1:] == lines[1][1:], lines                  # the timers' build of the path decides what the production path decides
    assert all(int(ln[3]) == 6 for ln in lines), lines          # the block resolver decided every batch
    assert [int(ln[4]) for ln in lines] == [ROUNDS["rr"], ROUNDS["rr"], ROUNDS["major"], ROUNDS["dense"]], lines   # the change moves no round
    blocks = re.findall(r"k_resolve6 tasks \[0, 3000\): \d+ rounds of (\d+) ", r.stderr)
    assert blocks == ["1408"], r.stderr[-3000:]                 # (the one run that reports)
    assert re.search(r"the stops \d+, a group's epilogue", r.stderr), r.stderr[-3000:]   # the walk timer's split is reported
    assert re.search(r"^ahead-child: what=volumes placed=\d+ resolver=6$", r.stdout, re.M), r.stdout
