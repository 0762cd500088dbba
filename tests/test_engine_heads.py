"""GPU: the commit kernel's matcher reading a group's set-up from LDS only (swp_resolve6.hpp, r6_commit_t: task flags in the L_cur words,
descriptor ids in the pick slots) against the CPU oracle, in the manner of tests/test_engine_window.py: 3 000 cfg3 tasks on 4 096 nodes,
each run a process of its own under its own time limit, chained so that nothing starts on the device behind a run that failed —
round-robin in blocks of 1 408 (no run of identical tasks: the engine tells the kernel to leave the run path alone), once as in
production and once with the section timers' report on (for the block size it prints); service-major as
the engine runs it (windows of 32 in blocks of 768); service-major with that policy off (runs by rank from 16-entry windows in blocks
of 1 408); and a batch with cluster mounts (k_r6_commit_v) on the volume script the smoke run uses. Placements and the explanations of
the unplaceable tasks equal the oracle's. The CPU side, with every path counted: tests/test_emu_resolve6_heads.py."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "heads_gpu_child.py")


def test_heads_from_lds_match_the_oracle():
    py = sys.executable
    cmd = ("timeout -k 10 120 env SWP_R6_BLOCK=1408 {py} {c} rr && "
           "timeout -k 10 120 env SWP_R6_BLOCK=1408 SWP_DBG=16 {py} {c} rr && "
           "timeout -k 10 120 {py} {c} major && "
           "timeout -k 10 120 env SWP_R6_RUNS=0 SWP_DBG=16 {py} {c} major && "
           "timeout -k 10 120 {py} {c} volumes").format(py=py, c=CHILD)
    env = {k: v for k, v in os.environ.items() if k not in ("SWP_R6_BLOCK", "SWP_DBG", "SWP_R6_RUNS", "SWP_R6_TWINS")}
    r = subprocess.run(["bash", "-c", cmd], capture_output=True, text=True, env=env)
    print(r.stdout[-3000:])
    print(r.stderr[-3000:])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = re.findall(r"^heads-child: what=(\w+) placed=(\d+) unplaceable=(\d+) resolver=(\d+) rounds=(\d+)$", r.stdout, re.M)
    assert [ln[0] for ln in lines] == ["rr", "rr", "major", "major"], r.stdout
    assert lines[0][1:] == lines[1][1:], lines                  # the timers' build of the path decides what the production path decides
    assert all(int(ln[3]) == 6 for ln in lines), lines          # the block resolver decided every batch
    assert lines[2][1:3] == lines[3][1:3], lines                # the runs policy changes the rounds, never the outcome
    blocks = re.findall(r"k_resolve6 tasks \[0, 3000\): \d+ rounds of (\d+) ", r.stderr)
    assert blocks == ["1408", "1408"], r.stderr[-3000:]         # (the two runs that report)
    assert re.search(r"^heads-child: what=volumes placed=\d+ resolver=6$", r.stdout, re.M), r.stdout
