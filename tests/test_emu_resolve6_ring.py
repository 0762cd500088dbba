"""CPU: the block resolver's ring rounds (swarmkit_amd/csrc/swp_resolve6.hpp, R6Args.ring, k_r6_commit_r) — the kernels' own source on
fibers (tests/emu/wv_emu.hpp) against the sequential model (tests/emu/emu_resolve6_ring.cpp): behind every round the placements of the
tasks it decided, at the end the whole state. Blocks are longer than the ring of fifteen 64-task slots, so slots are reused. The driver
REPORTS what a run came across ("reach ring: ..."): every case below asserts the path it is there for. Two builds: the tree's, and
-DR6_RING_ON=0 (the ring compiled out), which runs with the ring off are compared with commit launch by commit launch.
The GPU side: tests/test_engine_ring.py."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
CSRC = os.path.join(HERE, "..", "swarmkit_amd", "csrc")
BINS = {1: os.path.join(HERE, "_build", "emu_resolve6_ring"), 0: os.path.join(HERE, "_build", "emu_resolve6_ring_off"),
        "san": os.path.join(HERE, "_build", "emu_resolve6_ring_san")}


@pytest.fixture(scope="module")
def emu_bins():
    srcs = [os.path.join(EMU, "emu_resolve6_ring.cpp"), os.path.join(EMU, "wv_emu.hpp"), os.path.join(EMU, "emu_model.hpp"),
            os.path.join(CSRC, "swp_resolve6.hpp"), os.path.join(CSRC, "swp_shard.hpp"), os.path.join(CSRC, "swp_types.hpp"),
            os.path.join(CSRC, "swp_volumes.hpp")]
    flags = {1: ["-O2"], 0: ["-O2", "-DR6_RING_ON=0"], "san": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
    for key, path in BINS.items():
        os.makedirs(os.path.dirname(path), exist_ok=True)
        if not os.path.exists(path) or any(os.path.getmtime(s) > os.path.getmtime(path) for s in srcs):
            tmp = path + ".%d.tmp" % os.getpid()   # (xdist workers may build at the same time)
            subprocess.run(["g++", "-std=c++17"] + flags[key] + ["-o", tmp, srcs[0]], check=True)
            os.replace(tmp, path)
    return BINS


def run(bins, key, seed, shape, order, feat, *opts, lvl="0", sched=None):
    e = dict(os.environ)
    e.pop("EMU_SCHED_SEED", None)
    e.pop("EMU_LVL_MODE", None)
    if lvl is not None:
        e["EMU_LVL_MODE"] = lvl
    if sched:
        e["EMU_SCHED_SEED"] = str(sched)   # the fibers' waves in a seeded random order instead of first in, first out
    n, t, s, b = shape
    r = subprocess.run([bins[key]] + [str(x) for x in (seed, n, t, s, b, order, feat)] + ["v"] + list(opts), capture_output=True, text=True, timeout=900, env=e)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "-> OK" in r.stderr
    m = re.search(r"^reach ring: (.*)$", r.stderr, re.M)
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", m.group(1))}, r.stdout


SCHEDS = pytest.mark.parametrize("sched", [None, 17, 29, 101], ids=["fifo", "sched17", "sched29", "sched101"])


@SCHEDS
def test_block_1088_reuses_slots_0_and_1(emu_bins, sched):
    """Seventeen groups: groups 15 and 16 live in the slots of groups 0 and 1. Lists of up to 128 entries with a second section.
    (Every schedule of the waves: the hand-over of a slot between the matcher and its helper must hold whoever runs first.)"""
    got, _ = run(emu_bins, 1, 1, (4160, 7000, 70, 1088), 0, 0, sched=sched)
    assert got["ring"] == 960 and got["list"] == 128, got
    assert got["slot_reused"] > 0 and got["slots_reused_twice"] == 0 and got["wrapped_stages"] > 0, got
    assert got["long_lists"] > 0 and got["long_sections"] > 0 and got["crossed_wrapped"] > 0, got
    assert got["rounds"] == 7, got   # ceil(7 000 / 1 088): no round was cut


@SCHEDS
def test_block_1984_reuses_every_slot_one_of_them_twice(emu_bins, sched):
    """Thirty-one groups: every slot reused, slot 0 twice; the batch's last block ends on a short group; a cut at an exhausted list in
    a wrapped group; stagings that skip three and more dead batches of sixteen (how many depends on when a helper stages: asserted
    under the first-in-first-out schedule only)."""
    got, _ = run(emu_bins, 1, 1, (4160, 7000, 70, 1984), 0, 0, sched=sched)
    assert got["slot_reused"] > 0 and got["slots_reused_twice"] > 0, got
    assert got["short_last_group"] > 0 and got["cut_exhausted_wrapped"] + got["cut_window_wrapped"] > 0, got
    if sched is None:
        assert got["cut_exhausted_wrapped"] > 0 and got["skipped3"] > 0, got


def test_block_2816_picks_list_entries_beyond_64(emu_bins):
    """The production block on 8 256 nodes: picks out of list entries 64 and beyond, stagings that skip 3+ dead batches."""
    got, _ = run(emu_bins, 1, 2, (8256, 9000, 70, 2816), 0, 0)
    assert got["slots_reused_twice"] > 0 and got["picked_ge64"] > 0 and got["skipped3"] > 0, got
    assert got["rounds"] == 4, got


def test_levels_run_out_on_a_few_dozen_nodes_and_uneven_levels(emu_bins):
    """96 nodes, 4 services: after a lap every task must use its exception list — rounds of one task, each the block's first. And 2 112
    nodes on levels 0 to 2: cuts at exhausted lists inside wrapped groups."""
    got, _ = run(emu_bins, 1, 1, (96, 1200, 4, 1088), 0, 0)
    assert got["first_exc"] > 0 and got["cut_exhausted"] > 0, got
    got, _ = run(emu_bins, 1, 2, (2112, 6000, 40, 1984), 0, 0, lvl="1")
    assert got["cut_exhausted_wrapped"] > 0 and got["slot_reused"] > 0, got


@SCHEDS
def test_cut_at_a_window_in_a_wrapped_group(emu_bins, sched):
    """Windows of 8 entries: a block is cut in a wrapped group. (Whether a window runs out depends on when its helper staged it; under
    a random schedule the cut may be one at an exhausted list instead — a cut in a wrapped group it is.)"""
    got, _ = run(emu_bins, 1, 5, (4160, 7000, 70, 1984), 0, 0, "W8", sched=sched)
    assert got["cut_window_wrapped"] + got["cut_exhausted_wrapped"] > 0, got
    if sched is None:
        assert got["cut_window_wrapped"] > 0, got


@pytest.mark.parametrize("sched", [None, 17], ids=["fifo", "sched17"])
def test_uncounted_and_exception_tasks_in_wrapped_groups(emu_bins, sched):
    """Every 1 500th task uncounted: the block ends behind it, in group 23. Task 1 500 with no plain candidate: the block is cut in
    front of it (group 23) and the next round takes it from its exception list as its first task."""
    got, _ = run(emu_bins, 1, 1, (4160, 7000, 70, 1984), 0, 0, "U1500", sched=sched)
    assert got["cut_uncounted_wrapped"] > 0, got
    got, _ = run(emu_bins, 1, 1, (4160, 7000, 70, 1984), 0, 0, "E1500", sched=sched)
    assert got["cut_exception_wrapped"] > 0 and got["first_exc"] > 0, got


@pytest.mark.parametrize("seed,order,feat,shape", [(1, 0, 0, (4160, 7000, 70, 1408)), (3, 2, 2, (4160, 2400, 70, 256)), (2, 1, 0, (2304, 2560, 127, 1408))],
                         ids=["rr", "random-feat2", "major"])
def test_ring_off_is_the_build_without_the_ring(emu_bins, seed, order, feat, shape):
    """R6Args.ring = 0 against the build with the ring compiled out, same seed, launch by launch: accepted tasks, reason of the cut,
    seating steps, stops, the control block's counters and the pick slots (folded) of every commit launch."""
    a, out_a = run(emu_bins, 1, seed, shape, order, feat, "r0", "R", lvl=None)
    b, out_b = run(emu_bins, 0, seed, shape, order, feat, "R", lvl=None)
    ra, rb = re.findall(r"^round: .*$", out_a, re.M), re.findall(r"^round: .*$", out_b, re.M)
    assert len(ra) >= 1 and ra == rb, (len(ra), len(rb))
    assert a["ring"] == 0 and b["ring"] == 0 and a["list"] == 64 and a["rounds"] == b["rounds"], (a, b)


def test_under_address_and_undefined_behaviour_sanitizers(emu_bins):
    """The stand-alone driver (its own main) built with -fsanitize=address,undefined: a wrapped block with an exception task."""
    got, _ = run(emu_bins, "san", 1, (4160, 4000, 70, 1088), 0, 0, "E1500")
    assert got["slot_reused"] > 0, got


def test_fuzz_8_seeds_under_two_schedules_equal_the_model(emu_bins):
    """8 drawn shapes, each twice (first in first out, and a seeded random schedule of the waves) (N of 2 112 / 4 160 / 8 256, blocks of 1 088 / 1 472 / 1 984 / 2 816, every order, features 0 to 3, task rows,
    short windows, no twins), each against the model; sixteen plain processes side by side, a seed each (a batch with heavy services
    or uncounted tasks takes hundreds of rounds, each proposing a whole block: a minute or two of one core)."""
    env = dict(os.environ)
    env.pop("EMU_LVL_MODE", None)
    envs = []
    for k in range(16):   # seeds 1..8 first in, first out; the same eight again under a random schedule of the waves each
        e = dict(env)
        e.pop("EMU_SCHED_SEED", None)
        if k >= 8:
            e["EMU_SCHED_SEED"] = str(100 + k)
        envs.append(e)
    procs = [subprocess.Popen([emu_bins[1], "fuzz", str(1 + k % 8), "1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=envs[k]) for k in range(16)]
    outs = [p.communicate(timeout=3000) for p in procs]
    tot = {}
    for p, (out, err) in zip(procs, outs):
        assert p.returncode == 0, (out[-1500:], err[-1500:])
        assert "1 seeds, 0 failed" in out, out[-500:]
        m = re.search(r"^reach ring: (.*)$", err, re.M)
        for k, v in re.findall(r"(\w+)=(\d+)", m.group(1)):
            tot[k] = tot.get(k, 0) + int(v)
    assert tot["slot_reused"] > 0 and tot["long_lists"] > 0 and tot["wrapped_stages"] > 0, tot
