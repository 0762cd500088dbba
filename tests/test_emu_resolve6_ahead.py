"""CPU: the matcher's entries requested ahead of its cursor (swarmkit_amd/csrc/swp_resolve6.hpp, r6_commit_t, R6_SEAT_AHEAD) on fibers
(tests/emu/wv_emu.hpp). tests/emu/emu_resolve6_ahead.cpp is ONE program of two objects: the product headers, the model and the drivers
emu_resolve6_heads.cpp / emu_resolve7.cpp compiled with the switch off and with it on, each in a namespace of its own. Every case runs
under both builds from the same state and the same wave order; the program requires both to agree with the sequential model, the two
records to be equal launch by launch — the accepted tasks, the reason of the cut, the seating steps, the stops, the pick slots (node,
commit index, exception-list entry) of every accepted task, Blk6.rounds / reseats / cut_exhausted / cut_window / cut_exception /
cut_uncounted — and the paths a case is there for to have been reached (the kernel's R6_REACH hook counts them): it exits non-zero
otherwise, and a path that no case reached fails the run of all cases. Sizes: at most 256 nodes and 400 tasks.
(The two objects both carry wv_emu.hpp's context switch, a global symbol defined in a top-level asm: linked with -z muldefs, the
definitions are the same bytes.) The GPU side: tests/test_engine_ahead.py."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
CSRC = os.path.join(HERE, "..", "swarmkit_amd", "csrc")
BIN = os.path.join(HERE, "_build", "emu_resolve6_ahead")

CASES = ["stops_rr", "stops_lvl5", "window_3_entries", "window_1_entry", "features_2_blocks_of_64", "features_2_blocks_of_256", "mounts",
         "runs_major", "runs_major_win32", "compact", "compact_fused", "r7_3_shards", "r7_mounts"]
# what each case must have met (the program checks the same: stated here for the reader)
NEED = {
    "stops_rr": ["group_with_3_stops", "stop_with_idle_lanes", "cursor_at_list_end", "group_below_64_tasks"],
    "stops_lvl5": ["group_with_3_stops", "stop_with_idle_lanes"],
    "window_3_entries": ["read_clamped_at_window_end", "cursor_at_list_end"],
    "window_1_entry": ["window_of_one_entry", "read_clamped_at_window_end"],
    "features_2_blocks_of_64": ["first_task_from_exception_list"],
    "features_2_blocks_of_256": ["uncounted_task", "stop_with_idle_lanes"],
    "mounts": ["mounts_task"],
    "runs_major": ["group_behind_run_prefix", "second_seating_step"],
    "runs_major_win32": ["group_behind_run_prefix"],
    "compact": ["compact_index_round"],
    "compact_fused": ["compact_index_round"],
    "r7_3_shards": ["r7_instance", "group_with_3_stops"],
    "r7_mounts": ["r7_instance", "mounts_task"],
}


@pytest.fixture(scope="module")
def emu_bin():
    srcs = [os.path.join(EMU, f) for f in ("emu_resolve6_ahead.cpp", "emu_resolve6_heads.cpp", "emu_resolve7.cpp", "wv_emu.hpp", "emu_model.hpp")] + \
           [os.path.join(CSRC, f) for f in ("swp_resolve6.hpp", "swp_resolve7.hpp", "swp_shard.hpp", "swp_types.hpp", "swp_volumes.hpp")]
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    if not os.path.exists(BIN) or any(os.path.getmtime(s) > os.path.getmtime(BIN) for s in srcs):
        tmp = BIN + ".%d.tmp" % os.getpid()   # (xdist workers may build at the same time)
        objs = []
        for v in (0, 1):
            objs.append("%s.%d.o" % (tmp, v))
            subprocess.run(["g++", "-O2", "-std=c++17", "-DAHEAD_V=%d" % v, "-c", "-o", objs[-1], srcs[0]], check=True)
        subprocess.run(["g++", "-Wl,-z,muldefs", "-o", tmp] + objs, check=True)
        for o in objs:
            os.remove(o)
        os.replace(tmp, BIN)
    return BIN


def run(binary, case, sched=None):
    e = dict(os.environ)
    e.pop("EMU_SCHED_SEED", None)
    e.pop("EMU_LVL_MODE", None)
    if sched:
        e["EMU_SCHED_SEED"] = str(sched)
    r = subprocess.run([binary, case], capture_output=True, text=True, timeout=600, env=e)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    m = re.search(r"^ahead case %s: OK (.*)$" % case, r.stdout, re.M)
    assert m, r.stdout[-2000:]
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", m.group(1))}


def test_the_case_list_is_the_programs(emu_bin):
    r = subprocess.run([emu_bin, "list"], capture_output=True, text=True, timeout=60)
    assert r.stdout.split() == CASES and sorted(NEED) == sorted(CASES)
    # every path the issue names is asked of some case
    asked = {p for v in NEED.values() for p in v}
    assert asked == {"group_with_3_stops", "stop_with_idle_lanes", "second_seating_step", "cursor_at_list_end", "read_clamped_at_window_end", "window_of_one_entry",
                     "group_below_64_tasks", "first_task_from_exception_list", "uncounted_task", "mounts_task", "group_behind_run_prefix", "compact_index_round", "r7_instance"}


@pytest.mark.parametrize("case", CASES)
def test_switch_on_equals_switch_off_and_the_model(emu_bin, case):
    got = run(emu_bin, case)
    assert got["launches"] >= 1, got
    for path in NEED[case]:
        assert got[path] >= 1, (path, got)


@pytest.mark.parametrize("case", ["stops_rr", "runs_major", "r7_3_shards"])
def test_under_a_seeded_random_wave_order(emu_bin, case):
    """EMU_SCHED_SEED: the next wave to run is drawn at random where a wave is of one mind — the helpers stage, move cursors and apply at
    other moments than in the first-in-first-out order; both builds get the same draw."""
    got = run(emu_bin, case, sched=21)
    assert got["launches"] >= 1, got
