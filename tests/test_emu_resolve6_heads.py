"""CPU: the hand-over of the task heads through LDS in the block resolver's commit kernel (swarmkit_amd/csrc/swp_resolve6.hpp, r6_commit_t)
on fibers (tests/emu/wv_emu.hpp) against the sequential model. The wave that stages a group's windows leaves every task's flags in its
L_cur word and its descriptor id in its pick slot; wave 0 reads a group's set-up from LDS only. tests/emu/emu_resolve6_heads.cpp is the
window driver with a "reach heads:" line that counts what a run met in groups >= 2 of a round — the groups a HELPER staged: every case
below asserts the path it is there for. FIFO and seeded random wave orders (EMU_SCHED_SEED): a race in the hand-over shows there.
The GPU side: tests/test_engine_heads.py.

The model's own shapes meet two of the cuts only in a round's first two groups — a service runs out of plain nodes when it has many
tasks, which then follow each other closely, and the `feat 2` shape's blocks of 64 tasks have one group — so the driver forces them
into late groups: option E (the last service already runs on every node: its tasks, one every S, have only an exception-list
candidate) and option U<k> (exactly every k-th task is uncounted). The cases run the production path; those marked P run with the
kernel's section timers on (R6Args.dbg bit 4), which also report the picks the runs-by-rank path took in groups >= 2."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
CSRC = os.path.join(HERE, "..", "swarmkit_amd", "csrc")
BIN = os.path.join(HERE, "_build", "emu_resolve6_heads")


@pytest.fixture(scope="module")
def emu_bin():
    srcs = [os.path.join(EMU, "emu_resolve6_heads.cpp"), os.path.join(EMU, "wv_emu.hpp"), os.path.join(EMU, "emu_model.hpp"),
            os.path.join(CSRC, "swp_resolve6.hpp"), os.path.join(CSRC, "swp_shard.hpp"), os.path.join(CSRC, "swp_types.hpp"),
            os.path.join(CSRC, "swp_volumes.hpp")]
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    if not os.path.exists(BIN) or any(os.path.getmtime(s) > os.path.getmtime(BIN) for s in srcs):
        tmp = BIN + ".%d.tmp" % os.getpid()   # (xdist workers may build at the same time)
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", tmp, srcs[0]], check=True)
        os.replace(tmp, BIN)
    return BIN


def run(binary, case, env=None, sched=None):
    e = dict(os.environ)
    e.pop("EMU_SCHED_SEED", None)
    e.update(env or {})
    if sched:
        e["EMU_SCHED_SEED"] = str(sched)
    r = subprocess.run([binary] + [str(x) for x in case[:7]] + ["v"] + list(case[7:]), capture_output=True, text=True, timeout=600, env=e)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "-> OK" in r.stderr
    got = {}
    for line in ("window", "heads", "mounts"):
        m = re.search(r"^reach %s: (.*)$" % line, r.stderr, re.M)
        if m:
            got.update({k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", m.group(1))})
    cuts = re.search(r"cut: exhausted (\d+) exception (\d+) uncounted (\d+)", r.stderr)
    got["cut_exception"], got["cut_uncounted"] = int(cuts.group(2)), int(cuts.group(3))
    got["model_rounds"] = int(re.search(r"rounds (\d+) \(", r.stderr).group(1))
    return got


FLAT = {"EMU_LVL_MODE": "0"}   # every node on one level: lists as long as they get, rounds that fill their block
SCHEDS = pytest.mark.parametrize("sched", [None, 21], ids=["fifo", "sched21"])

# (seed, nodes, tasks, services, block, task order, feature level, options...)
TWO_GROUPS = (101, 8192, 3000, 400, 1408, 0, 0)


@SCHEDS
def test_a_helper_leaves_the_heads_of_a_second_group(emu_bin, sched):
    """Rounds that decide more than 960 tasks: helper h leaves flags and descriptor ids for group h + 15 in pick slots next to those it
    has just applied from. The shape has unplaceable tasks (level == R6_NONE, no exception candidate) in late groups: decided from the flags."""
    got = run(emu_bin, TWO_GROUPS, FLAT, sched)
    assert got["block"] == 1408 and got["rounds_two_groups"] >= 2, got
    assert got["late_unplaceable"] >= 100, got


@SCHEDS
def test_no_runs_flag_skips_the_run_path_only(emu_bin, sched):
    """R6Args.no_runs (the engine: a batch without a run of >= 8 identical tasks): no descriptor id is left or read, same outcome."""
    got = run(emu_bin, TWO_GROUPS + ("R",), FLAT, sched)
    assert got["no_runs"] == 1 and got["rounds_two_groups"] >= 2, got
    # service-major: groups that start with a run of identical tasks are there, the path is not taken, the outcome is the model's
    got = run(emu_bin, (103, 8192, 3000, 12, 1408, 1, 0, "R", "P"), FLAT, sched)
    assert got["no_runs"] == 1 and got["late_run_groups"] >= 20 and got["late_run_tasks"] == 0, got


@SCHEDS
def test_cut_behind_an_uncounted_task_in_a_late_group(emu_bin, sched):
    """Every 300th task is uncounted: each round is cut behind one (why 3) in a group >= 2, from the bit its helper left."""
    got = run(emu_bin, TWO_GROUPS + ("U300",), FLAT, sched)
    assert got["cut_uncounted"] == 10 and got["late_cut_uncounted"] == 10 and got["model_rounds"] == 10, got


@SCHEDS
def test_cut_in_front_of_an_exception_list_task_in_a_late_group(emu_bin, sched):
    """Option E, 400 services in round-robin order: the tasks 399, 799, ... have no plain candidate (level == R6_NONE) but an exception-list
    candidate. Each sits in a group >= 2 of its round, staged by a helper: the round is cut in front of it (why 2) from the R6C_EXC bit
    the helper left — a lost bit would make the task unplaceable and the outcome differ from the model's — and the next round places it
    first, from thread 0's record. No mounts in the batch: every why-2 cut is an exception-list cut."""
    got = run(emu_bin, TWO_GROUPS + ("E",), FLAT, sched)
    assert got["late_cut_exception"] == 7 and got["first_from_exception_list"] == 7 and got["late_cut_mount"] == 0, got
    assert got["timers"] == 0, got


@SCHEDS
def test_feature_level_2_in_blocks_of_64(emu_bin, sched):
    """The existing `feat 2` shape (host ports, uncounted tasks, exception lists, random order, blocks of one group): the prologue's flags,
    and the block's first task from its exception list (thread 0 keeps its record)."""
    got = run(emu_bin, (3, 1000, 2500, 40, 64, 2, 2), None, sched)
    assert got["cut_uncounted"] >= 20 and got["cut_exception"] >= 10 and got["first_from_exception_list"] >= 5, got


@SCHEDS
def test_cut_in_front_of_an_exception_list_task(emu_bin, sched):
    """Blocks of 1 408: rounds cut in front of a task that must use its exception list (why 2), which the next round places first."""
    got = run(emu_bin, (4, 4096, 2000, 20, 1408, 0, 1), FLAT, sched)
    assert got["cut_exception"] >= 6 and got["first_from_exception_list"] >= 3 and got["late_unplaceable"] >= 50, got


@SCHEDS
def test_second_task_with_cluster_mounts_in_a_late_group(emu_bin, sched):
    """k_r6_commit_v, a task with mounts every 300 tasks: a round decides one and is cut in front of the next (why 2) in a group >= 2.
    (U5000: no task of the 1 500 is uncounted, so that feature level 4's uncounted services do not cut the rounds short. The driver
    tells a why-2 cut in front of a task with mounts from one in front of an exception-list task.)"""
    got = run(emu_bin, (34, 4096, 1500, 60, 1408, 0, 4, "m300", "U5000"), FLAT, sched)
    assert got["cut_at_second_mount"] >= 2 and got["late_cut_mount"] >= 2 and got["late_cut_exception"] == 0, got


@SCHEDS
def test_cluster_mounts_every_tenth_task(emu_bin, sched):
    """The existing `m10` shape on k_r6_commit_v: cuts in front of a second task with mounts (in the prologue's groups)."""
    got = run(emu_bin, (34, 1500, 500, 60, 1408, 0, 4, "m10", "a"), None, sched)
    assert got["with_attachments"] > 0 and got["cut_at_second_mount"] > 0 and got["cut_exception"] > 0, got


@SCHEDS
def test_compact_index_instance(emu_bin, sched):
    """k_r6_commit_c, the existing `c` shape: the same flags next to windows of compact positions."""
    got = run(emu_bin, (12, 5924, 1856, 377, 1408, 0, 0, "c"), {"EMU_LVL_MODE": "5"}, sched)
    assert got["compact_rounds"] >= 5, got


@pytest.mark.parametrize("case", [(103, 8192, 3000, 12, 1408, 1, 0, "P"), (103, 8192, 3000, 12, 768, 1, 0, "L32", "P")], ids=["block1408-win16", "block768-L32"])
@SCHEDS
def test_runs_by_rank_in_late_groups(emu_bin, case, sched):
    """Service-major order, 250 twins in a row: runs are taken by rank in groups >= 2, whose descriptor ids come from a helper's slots."""
    got = run(emu_bin, case, FLAT, sched)
    assert got["timers"] == 1 and got["late_run_tasks"] >= 500 and got["late_run_groups"] >= 20, got
    assert got["model_rounds"] <= 8, got
