"""CPU: the block resolver's lists over two levels (swarmkit_amd/csrc/swp_resolve6.hpp, r6_propose_t "the second section",
R6Args.levels2) — the kernels' own source on fibers (tests/emu/wv_emu.hpp) against the sequential model, and every proposal of every
round against the list rule restated on the host (tests/emu/emu_resolve6_levels.cpp). The driver REPORTS what a run came across
("reach levels: ..."): every case below asserts the path it is there for. Two builds: the tree's, and -DR6_LEVELS2=0 (the second
section compiled out: what the kernels were before), which runs with levels2 = 0 are compared with commit launch by commit launch.
The base shape: 2 304 nodes (72 half-words), 7 000 tasks of 70 services, blocks of 1 408 — three laps over the node set, so levels
run out inside blocks. The GPU side: tests/test_engine_levels.py."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
CSRC = os.path.join(HERE, "..", "swarmkit_amd", "csrc")
BINS = {1: os.path.join(HERE, "_build", "emu_resolve6_levels"), 0: os.path.join(HERE, "_build", "emu_resolve6_levels_off")}
BASE = (2304, 7000, 70, 1408)   # nodes, tasks, services, block


@pytest.fixture(scope="module")
def emu_bins():
    srcs = [os.path.join(EMU, "emu_resolve6_levels.cpp"), os.path.join(EMU, "wv_emu.hpp"), os.path.join(EMU, "emu_model.hpp"),
            os.path.join(CSRC, "swp_resolve6.hpp"), os.path.join(CSRC, "swp_shard.hpp"), os.path.join(CSRC, "swp_types.hpp"),
            os.path.join(CSRC, "swp_volumes.hpp")]
    for on, path in BINS.items():
        os.makedirs(os.path.dirname(path), exist_ok=True)
        if not os.path.exists(path) or any(os.path.getmtime(s) > os.path.getmtime(path) for s in srcs):
            tmp = path + ".%d.tmp" % os.getpid()   # (xdist workers may build at the same time)
            subprocess.run(["g++", "-O2", "-std=c++17"] + ([] if on else ["-DR6_LEVELS2=0"]) + ["-o", tmp, srcs[0]], check=True)
            os.replace(tmp, path)
    return BINS


def run(bins, on, seed, order, feat, *opts, shape=BASE, lvl="0", sched=None):
    e = dict(os.environ)
    e.pop("EMU_SCHED_SEED", None)
    e.pop("EMU_LVL_MODE", None)
    if lvl is not None:
        e["EMU_LVL_MODE"] = lvl
    if sched:
        e["EMU_SCHED_SEED"] = str(sched)
    n, t, s, b = shape
    r = subprocess.run([bins[on]] + [str(x) for x in (seed, n, t, s, b, order, feat)] + ["v"] + list(opts), capture_output=True, text=True, timeout=900, env=e)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "-> OK" in r.stderr
    m = re.search(r"^reach levels: (.*)$", r.stderr, re.M)
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", m.group(1))}, r.stdout


@pytest.mark.parametrize("sched", [None, 17], ids=["fifo", "sched17"])
def test_base_shape_crosses_levels_in_fewer_rounds(emu_bins, sched):
    """Round-robin, every node on one level at the start: second sections, sections cut by the room (bit 31), tasks placed one level
    above their record's in groups a helper staged, proposals beyond Blk6.maxrel and lists without room — and fewer rounds than
    with the switch off, never fewer than the batch has blocks. Under the timers' bit Blk6.dbg_lv2 counts the sections."""
    on, _ = run(emu_bins, 1, 1, 0, 0, "P", sched=sched)
    off, _ = run(emu_bins, 1, 1, 0, 0, "l0", sched=sched)
    assert on["levels2"] == 1 and off["levels2"] == 0 and off["sections"] == 0 and off["crossed"] == 0, (on, off)
    assert on["sections"] > 0 and on["truncated"] > 0 and on["crossed"] > 0 and on["crossed_in_late_group"] > 0, on
    assert on["beyond_maxrel"] > 0 and on["no_room"] > 0 and on["list_cut"] > 0, on
    assert on["dbg_lv2"] == on["sections"], on
    assert off["twins_use_level"] > 0, off   # (the twins' share >= the level's candidates: a one-entry list, a cut — met where the rounds are cut)
    assert (BASE[1] + BASE[3] - 1) // BASE[3] <= on["rounds"] < off["rounds"], (on, off)


@pytest.mark.parametrize("seed,order,feat,opts", [(1, 0, 0, ()), (2, 0, 3, ()), (3, 2, 1, ()), (2, 1, 0, ()), (4, 0, 0, ("x",))],
                         ids=["rr", "rr-feat3", "random-feat1", "major", "rr-no-ext"])
def test_switch_off_is_the_build_without_the_section(emu_bins, seed, order, feat, opts):
    """levels2 = 0 against the build with the second section compiled out, same seed, launch by launch: accepted tasks, reason of the
    cut, seating steps, stops, the control block's counters and the pick slots (folded) of every commit launch."""
    shape = BASE if feat == 0 else (2304, 1200, 70, 256)
    a, out_a = run(emu_bins, 1, seed, order, feat, "l0", "R", *opts, shape=shape, lvl=None)
    b, out_b = run(emu_bins, 0, seed, order, feat, "R", *opts, shape=shape, lvl=None)
    ra, rb = re.findall(r"^round: .*$", out_a, re.M), re.findall(r"^round: .*$", out_b, re.M)
    assert len(ra) >= 1 and ra == rb, (len(ra), len(rb))
    assert a["sections"] == 0 and b["sections"] == 0 and a["rounds"] == b["rounds"], (a, b)


def test_features_uncounted_first_word_twins_and_short_windows(emu_bins):
    """Features 0 to 3 on uneven levels (the model's default draw): an uncounted task in front of tasks with a second section (the
    block ends behind it), levels whose first candidate sits in word 0 (no section), twins that use their level up (a one-entry list)
    and a short window over lists with second sections."""
    tot = {}
    for seed in (1, 2, 3):
        got, _ = run(emu_bins, 1, seed, 0, 3, shape=(2304, 1500, 70, 256), lvl=None)
        for k, v in got.items():
            tot[k] = tot.get(k, 0) + v
    assert tot["sections"] > 0 and tot["crossed"] > 0, tot
    assert tot["uncounted_before_section"] > 0 and tot["first_word"] > 0 and tot["twins_use_level"] > 0 and tot["nothing_in_front"] > 0, tot
    got, _ = run(emu_bins, 1, 5, 0, 0, "W4", shape=(2304, 7000, 70, 1408), lvl="1")
    assert got["sections"] > 0 and got["window_cuts"] > 0, got


def test_block_cut_at_an_exhausted_second_section(emu_bins):
    """A cut with the reason "exhausted" (Blk6.cut_exhausted, not a window that ran out) at a task whose list has a second section:
    the driver checks for every such cut that every node the list names, first and second section alike, was taken by the round's
    tasks in front of it — it fails on a free one — and counts the cuts at lists with a second section. 2 112 nodes on levels
    0 to 2, 4 000 tasks of 40 services."""
    got, _ = run(emu_bins, 1, 2, 0, 0, shape=(2112, 4000, 40, 1408), lvl="1")
    assert got["cut_dry_section"] > 0, got
    assert got["cut_exhausted"] >= got["cut_dry_section"] and got["sections"] > 0 and got["crossed"] > 0, got


def test_task_rows_short_window_no_extension_and_mounts(emu_bins):
    got, _ = run(emu_bins, 1, 1, 0, 0, "t")
    assert got["sections_task_rows"] > 0 and got["crossed"] > 0, got
    got, _ = run(emu_bins, 1, 1, 0, 0, "W4")
    assert got["sections"] > 0 and got["crossed"] > 0, got
    got, _ = run(emu_bins, 1, 1, 0, 0, "x")   # R6Args.ext == nullptr: lists of 32, the section in what the first leaves of them
    assert got["list"] == 32 and got["sections"] > 0, got
    got, _ = run(emu_bins, 1, 34, 0, 4, "m10", "a", shape=(2304, 1500, 60, 256), lvl=None)   # tasks with cluster mounts get no section (the driver fails on one)
    assert got["mounts_no_section"] > 0 and got["sections"] > 0, got


def test_service_major_runs_cross_through_the_first_lanes_list(emu_bins):
    """Service-major: the runs-by-rank path hands a run's tasks the free candidates of its first task's list in list order — through
    the first section into the second."""
    got, _ = run(emu_bins, 1, 2, 1, 0, shape=(2304, 2560, 127, 1408), lvl=None)
    assert got["sections"] > 0 and got["crossed"] > 0, got


def test_fuzz_200_seeds_equal_the_model(emu_bins):
    """200 drawn shapes (N of 2 112 / 2 304 / 4 160, T <= 8 000, orders rr / major / random, features 0 to 4, task rows, no
    extension, short windows), each against the model and the restated rule; eight processes side by side (about six seconds of one
    core a seed)."""
    procs = [subprocess.Popen([emu_bins[1], "fuzz", str(1 + 25 * k), "25"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for k in range(8)]
    outs = [p.communicate(timeout=3000) for p in procs]
    tot = {}
    for p, (out, err) in zip(procs, outs):
        assert p.returncode == 0, (out[-1500:], err[-1500:])
        assert "25 seeds, 0 failed" in out, out[-500:]
        m = re.search(r"^reach levels: (.*)$", err, re.M)
        for k, v in re.findall(r"(\w+)=(\d+)", m.group(1)):
            tot[k] = tot.get(k, 0) + int(v)
    # the drawn shapes still reach what the fuzz is there for
    assert tot["sections"] > 0 and tot["truncated"] > 0 and tot["crossed"] > 0 and tot["mounts_no_section"] > 0 and tot["sections_task_rows"] > 0, tot
