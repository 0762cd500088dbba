"""The rule that cuts a batch's one-off tasks into spread segments (swarmkit_amd/csrc/swp_rounds.hpp spread_segments) without a GPU:
tests/emu/emu_spread_segs.cpp includes the header alone and prints the pieces for a string of task kinds.

The rule, restated: a segment starts at a task with preferences ('s'); it ends in front of a task the spread kernel cannot take ('m'),
or behind its last task with preferences that is followed by SPREAD_GAP = 64 or more tasks without ('.'), or at the end of the range —
fewer plain tasks than that between two tasks with preferences, or behind the last one up to the range's end, ride along. The pieces
tile the range in order. The expected pieces below are worked out by hand from that text.
TEST INFRASTRUCTURE around product source; no product code path uses it."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
CSRC = os.path.join(HERE, "..", "swarmkit_amd", "csrc")
BIN = os.path.join(HERE, "_build", "emu_spread_segs")


@pytest.fixture(scope="module")
def emu_bin():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    srcs = [os.path.join(EMU, "emu_spread_segs.cpp"), os.path.join(CSRC, "swp_rounds.hpp")]
    if not os.path.exists(BIN) or any(os.path.getmtime(s) > os.path.getmtime(BIN) for s in srcs):
        tmp = BIN + ".%d.tmp" % os.getpid()   # (xdist workers may build at the same time)
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", tmp, srcs[0]], check=True)
        os.replace(tmp, BIN)
    return BIN


def pieces(emu_bin, kinds, *rng):
    r = subprocess.run([emu_bin, kinds] + [str(x) for x in rng], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1].split()[0] == "segments" and lines[-1].split()[3] == "64"
    out = [tuple(int(x) for x in l.split()) for l in lines[:-1]]
    assert int(lines[-1].split()[1]) == sum(1 for p in out if p[2])
    return out


CASES = [
    ("10.", [(0, 10, 0)]),                                   # no task with preferences: one piece, no segment
    ("s", [(0, 1, 1)]),
    ("5s", [(0, 5, 1)]),
    ("3.s", [(0, 3, 0), (3, 1, 1)]),                         # a segment STARTS at a task with preferences
    ("s63.", [(0, 64, 1)]),                                  # a short tail rides along to the end of the range
    ("s64.", [(0, 1, 1), (1, 64, 0)]),                       # 64 plain tasks: the segment ends behind its last task with preferences
    ("s63.s", [(0, 65, 1)]),                                 # 63 between two: they ride along
    ("s64.s", [(0, 1, 1), (1, 64, 0), (65, 1, 1)]),          # 64 between two: two segments
    ("s10.s100.s", [(0, 12, 1), (12, 100, 0), (112, 1, 1)]),
    ("s3.ms", [(0, 1, 1), (1, 4, 0), (5, 1, 1)]),            # a task the kernel cannot take is never inside: the plain tasks in front of it stay out, too
    ("sm", [(0, 1, 1), (1, 1, 0)]),
    ("ms", [(0, 1, 0), (1, 1, 1)]),
    ("s130.40s200.31s", [(0, 1, 1), (1, 130, 0), (131, 40, 1), (171, 200, 0), (371, 31, 1)]),
]


@pytest.mark.parametrize("kinds,want", CASES, ids=[c[0] for c in CASES])
def test_segment_rule(emu_bin, kinds, want):
    got = pieces(emu_bin, kinds)
    assert got == want
    at = 0
    for first, count, _ in got:   # the pieces tile the range
        assert first == at and count > 0
        at += count


def test_a_range_inside_the_batch(emu_bin):
    """A stretch between two runs of identical tasks: only [j0, j1) is cut, a task with preferences outside it is not looked at."""
    assert pieces(emu_bin, "s4.s4.s", 1, 9) == [(1, 4, 0), (5, 4, 1)]
