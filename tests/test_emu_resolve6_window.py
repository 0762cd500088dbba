"""CPU: the block resolver's kernel SOURCE with late-staged list windows (swarmkit_amd/csrc/swp_resolve6.hpp, r6_commit_t) on fibers
(tests/emu/wv_emu.hpp) against the sequential model — tests/emu/emu_resolve6_window.cpp, which also REPORTS the paths a run came across
("reach window: ..."): every case below asserts the path it is there for. Two builds: the default window, and -DR6_WIN=4 (windows that
run out with entries left). The GPU side: tests/test_engine_window.py."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
CSRC = os.path.join(HERE, "..", "swarmkit_amd", "csrc")
BINS = {16: os.path.join(HERE, "_build", "emu_resolve6_window"), 4: os.path.join(HERE, "_build", "emu_resolve6_window4")}


@pytest.fixture(scope="module")
def emu_bins():
    srcs = [os.path.join(EMU, "emu_resolve6_window.cpp"), os.path.join(EMU, "wv_emu.hpp"), os.path.join(EMU, "emu_model.hpp"),
            os.path.join(CSRC, "swp_resolve6.hpp"), os.path.join(CSRC, "swp_shard.hpp"), os.path.join(CSRC, "swp_types.hpp"),
            os.path.join(CSRC, "swp_volumes.hpp")]
    for win, path in BINS.items():
        os.makedirs(os.path.dirname(path), exist_ok=True)
        if not os.path.exists(path) or any(os.path.getmtime(s) > os.path.getmtime(path) for s in srcs):
            tmp = path + ".%d.tmp" % os.getpid()   # (xdist workers may build at the same time)
            subprocess.run(["g++", "-O2", "-std=c++17"] + (["-DR6_WIN=%d" % win] if win != 16 else []) + ["-o", tmp, srcs[0]], check=True)
            os.replace(tmp, path)
    return BINS


def run(bins, win, case, env=None):
    e = dict(os.environ)
    e.pop("EMU_SCHED_SEED", None)
    e.update(env or {})
    r = subprocess.run([bins[win]] + [str(x) for x in case[:7]] + ["v"] + list(case[7:]), capture_output=True, text=True, timeout=600, env=e)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "-> OK" in r.stderr
    m = re.search(r"^reach window: (.*)$", r.stderr, re.M)
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", m.group(1))}, r.stderr


FLAT = {"EMU_LVL_MODE": "0"}   # every node on one level: lists as long as they get, rounds that fill their block

# (seed, nodes, tasks, services, block, task order, feature level, options...)
TWO_GROUPS = (101, 8192, 3000, 400, 1408, 0, 0)


@pytest.mark.parametrize("sched", [None, 11], ids=["fifo", "sched11"])
def test_block_of_1408_a_helper_takes_two_groups(emu_bins, sched):
    """Rounds that decide more than 960 tasks: helper h applies group h and then stages, waits for and applies group h + 15. Lists
    reach into the extension. The second run draws the waves' order at random."""
    got, _ = run(emu_bins, 16, TWO_GROUPS, dict(FLAT, **({"EMU_SCHED_SEED": str(sched)} if sched else {})))
    assert got["block"] == 1408 and got["rounds_two_groups"] >= 2, got
    assert got["long_lists"] > 0 and got["longest"] == 64 and got["ext"] == 1, got


@pytest.mark.parametrize("sched", [None, 12], ids=["fifo", "sched12"])
def test_null_extension_and_a_cut_inside_a_late_group(emu_bins, sched):
    """R6Args.ext == nullptr: lists end with the proposal's 32 entries (what the shard drivers pass). With the default window those
    lists run out behind 960 tasks: the block is cut inside a group >= 15, the cut is counted, the next round decides the task."""
    got, _ = run(emu_bins, 16, (106, 8192, 3000, 300, 1408, 0, 0, "x"), dict(FLAT, **({"EMU_SCHED_SEED": str(sched)} if sched else {})))
    assert got["ext"] == 0 and got["long_lists"] == 0 and got["longest"] == 32, got
    assert got["cuts_late"] >= 1 and got["rounds_two_groups"] >= 1, got
    assert got["window_cuts"] >= 1 and got["window_cut_then_decided"] == got["window_cuts"], got


@pytest.mark.parametrize("win,case,env", [
    (4, (102, 4096, 1000, 200, 1408, 0, 0), FLAT),                       # -DR6_WIN=4
    (16, (107, 4096, 1000, 200, 1408, 0, 0, "W4"), FLAT),                # the same window through R6Args.dbg, production build
    (4, (3, 1000, 2500, 40, 64, 2, 2), {}),                             # host ports, uncounted tasks, random order, small blocks
    (4, (103, 8192, 2000, 12, 1408, 1, 0), dict(FLAT, EMU_SCHED_SEED="13")),   # service-major under a random wave order
], ids=["R6_WIN4", "dbgW4", "R6_WIN4-feat2", "R6_WIN4-major-sched13"])
def test_short_windows_run_out_and_the_next_round_decides(emu_bins, win, case, env):
    got, _ = run(emu_bins, win, case, env)
    assert got["win"] == 4, got
    assert got["long_lists"] > 0 or case[1] <= 32 * 32, got   # (1 000 nodes are 32 half-words: no list can be longer)
    assert got["window_cuts"] >= 5 and got["window_cut_then_decided"] == got["window_cuts"], got


def test_service_major_runs_read_a_window(emu_bins):
    """Service-major order: the runs-by-rank path takes a run's picks from the window of the run's first lane; a run longer than the
    window's free candidates goes on with the next lane's list. 250 twins in a row."""
    got, err = run(emu_bins, 16, (103, 8192, 3000, 12, 1408, 1, 0), FLAT)
    assert got["long_lists"] > 0 and got["window_cuts"] >= 1 and got["window_cut_then_decided"] == got["window_cuts"], got
    rounds = int(re.search(r"rounds (\d+) \(", err).group(1))
    assert rounds <= 8, err[-500:]   # (tasks one at a time, without the run path and the twins' offsets, would be cut every 16 tasks)


@pytest.mark.parametrize("sched", [None, 12], ids=["fifo", "sched12"])
def test_windows_of_32_for_batches_of_runs(emu_bins, sched):
    """R6Args.win = 32 in blocks of 768: what the engine gives a batch that is mostly runs of identical tasks. The LDS layout follows
    the argument; lists still reach into the extension, so a window of 32 is the first 32 LIVE entries of up to 64."""
    got, _ = run(emu_bins, 16, (103, 8192, 3000, 12, 768, 1, 0, "L32"), dict(FLAT, **({"EMU_SCHED_SEED": str(sched)} if sched else {})))
    assert got["win"] == 32 and got["block"] == 768 and got["long_lists"] > 0, got


def test_compact_index_instance(emu_bins):
    """k_r6_commit_c (and the index built at its end): positions in the windows, translated back by the helpers' apply."""
    got, _ = run(emu_bins, 16, (12, 5924, 1856, 377, 1408, 0, 0, "c"), {"EMU_LVL_MODE": "5"})
    assert got["compact_rounds"] >= 5, got
    got, _ = run(emu_bins, 4, (12, 5924, 900, 377, 1408, 0, 0, "f"), {"EMU_LVL_MODE": "5"})
    assert got["compact_rounds"] >= 5 and got["window_cuts"] >= 1, got


def test_batch_with_cluster_mounts(emu_bins):
    """k_r6_commit_v: the helpers' apply chooses and reserves volumes; the harness compares attachments and every volume's usage."""
    got, err = run(emu_bins, 16, (34, 1500, 500, 60, 1408, 0, 4, "m10", "a"))
    m = re.search(r"^reach mounts: (.*)$", err, re.M)
    mounts = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", m.group(1))}
    assert mounts["with_attachments"] > 0 and mounts["cut_at_second_mount"] > 0, mounts
    assert got["long_lists"] > 0, got
