"""GPU: the block resolver's ring rounds (swp_resolve6.hpp R6Args.ring, k_r6_commit_r; the rule: swp_rounds.hpp r6_ring) against the CPU
oracle, in the manner of tests/test_engine_heads.py: every run a process of its own under its own time limit, chained so that nothing
starts on the device behind a run that failed. The ring is forced (SWP_R6_RING=1) with a block of 1 088 — seventeen groups, so slots 0
and 1 of the fifteen are reused — on 3 000 cfg3 tasks on 4 096 nodes, as in production and with the section timers' report on, and
switched off (SWP_R6_RING=0) for the same outcome; on 1 200 tasks of 4 services on 96 nodes, where levels run out all the time and blocks
are cut; service-major and the volume script run without knobs: the ring is off by rule there (a batch of runs, cluster mounts) and
the report says so. Placements and the explanations of the unplaceable tasks equal the oracle's.
The CPU side, with every path counted: tests/test_emu_resolve6_ring.py; the rule: tests/test_rounds_ring_cpu.py."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "ring_gpu_child.py")


def test_ring_rounds_match_the_oracle():
    py = sys.executable
    cmd = ("timeout -k 10 120 env SWP_R6_RING=1 SWP_R6_BLOCK=1088 {py} {c} rr && "
           "timeout -k 10 120 env SWP_R6_RING=1 SWP_R6_BLOCK=1088 SWP_DBG=16 {py} {c} rr && "
           "timeout -k 10 120 env SWP_R6_RING=0 SWP_R6_BLOCK=1088 {py} {c} rr && "
           "timeout -k 10 120 env SWP_R6_RING=1 SWP_R6_BLOCK=1088 SWP_DBG=16 {py} {c} small && "
           "timeout -k 10 120 env SWP_DBG=16 {py} {c} major && "
           "timeout -k 10 120 env SWP_DBG=16 {py} {c} volumes").format(py=py, c=CHILD)
    env = {k: v for k, v in os.environ.items() if k not in ("SWP_R6_BLOCK", "SWP_DBG", "SWP_R6_RUNS", "SWP_R6_TWINS", "SWP_R6_RING", "SWP_R6_LEVELS")}
    r = subprocess.run(["bash", "-c", cmd], capture_output=True, text=True, env=env)
    print(r.stdout[-3000:])
    print(r.stderr[-6000:])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = re.findall(r"^ring-child: what=(\w+) placed=(\d+) unplaceable=(\d+) resolver=(\d+) rounds=(\d+)$", r.stdout, re.M)
    assert [ln[0] for ln in lines] == ["rr", "rr", "rr", "small", "major"], r.stdout
    assert lines[0][1:] == lines[1][1:], lines                  # the timers' build of the path decides what the production path decides
    assert lines[0][1:3] == lines[2][1:3], lines                # the ring changes the rounds, never the outcome
    assert all(int(ln[3]) == 6 for ln in lines), lines          # the block resolver decided every batch
    reports = re.findall(r"k_resolve6 blocks: flat (\d+), lists of (\d+) \| ring (on|off)(?:: blocks of (\d+) over a ring of (\d+) tasks, lists of (\d+))?", r.stderr)
    assert len(reports) >= 4, r.stderr[-3000:]
    assert reports[0] == ("1088", "64", "on", "1088", "960", "128"), reports     # rr with the timers: the report names the ring
    assert reports[1][2:] == ("on", "1088", "960", "128"), reports               # small
    assert all(rep[2] == "off" for rep in reports[2:]), reports                  # service-major, the volume script: off by rule
    assert re.search(r"^ring-child: what=volumes placed=\d+ resolver=6$", r.stdout, re.M), r.stdout
