"""CPU: k_waterfill (swarmkit_amd/csrc/swp_waterfill.hpp, the product file unchanged) run on fibers (tests/emu/wv_emu.hpp: 1024 of
them, the kernel's raw HIP spellings supplied by tests/emu/emu_waterfill.cpp) against a sequential model that places a run one task at
a time from the reference's text: eligibility, ResourceFilter, MaxReplicas, then the minimum by (failure class, svcCount,
ActiveTasksCount, node index) and NodeInfo.addTask. No phases, capacities or scans in the model. Every array the kernel can write —
placements, node rows, the exception bitmap and list, the commit log with its chains, the "no node" records, Ctl — starts poisoned and is
compared in full after every launch. The states are NOT fresh clusters: uneven task counts, exception entries with counts and failures
below / at / above MAX_FAILURES, holes in the lists, negative residuals, non-zero commit positions, the same service launched twice.
No GPU involved; the GPU parity is tests/test_engine_waterfill.py.

Every "reach" figure asserted below is counted by the MODEL's run (never taken from the kernel's output)."""
import functools
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
BIN = os.path.join(HERE, "_build", "emu_waterfill")
CSRC = os.path.join(HERE, "..", "swarmkit_amd", "csrc")


@pytest.fixture(scope="module")
def emu_bin():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    srcs = [os.path.join(EMU, "emu_waterfill.cpp"), os.path.join(EMU, "wv_emu.hpp"), os.path.join(EMU, "emu_model.hpp"),
            os.path.join(CSRC, "swp_waterfill.hpp"), os.path.join(CSRC, "swp_volumes.hpp"), os.path.join(CSRC, "swp_types.hpp")]
    if not os.path.exists(BIN) or any(os.path.getmtime(s) > os.path.getmtime(BIN) for s in srcs):
        tmp = BIN + ".%d.tmp" % os.getpid()   # (xdist workers may build at the same time)
        subprocess.run(["g++", "-O1", "-std=c++17", "-o", tmp, srcs[0]], check=True)
        os.replace(tmp, BIN)
    return BIN


@functools.lru_cache(maxsize=None)
def _run(binary, args, sched):
    env = dict(os.environ)
    env.pop("EMU_SCHED_SEED", None)
    if sched:
        env["EMU_SCHED_SEED"] = str(sched)
    r = subprocess.run([binary] + list(args), capture_output=True, text=True, timeout=900, env=env)
    return r.returncode, r.stderr


def run_ok(binary, *args, sched=0):
    rc, err = _run(binary, tuple(str(a) for a in args), sched)
    assert rc == 0, err[-3000:]
    assert "-> OK" in err, err[-3000:]
    return err


def reach(err):
    m = re.search(r"^reach waterfill: ?(.*)$", err, re.M)
    assert m, err[-2000:]
    print(m.group(0))
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", m.group(1))}


# (seed, nodes, run lengths). Nodes: one, two, around a wave (63, 64, 65), around one node per thread (1023, 1024, 1025: two nodes a thread
# and about half the threads empty-handed), around two (2047, 2049), three a thread with threads left over (3000). Lengths: 0 runs of 1 and 2;
# 1 about one lap of the eligible nodes; 2 several laps; 3 more than the cluster takes (the tail finds no node).
SEEDED = [(1, 1, 2), (2, 2, 2), (15, 2, 3), (3, 63, 2), (4, 64, 1), (5, 65, 3), (16, 65, 0), (6, 1023, 2), (7, 1024, 1), (17, 1024, 3), (8, 1025, 2), (13, 1025, 0),
          (18, 1025, 1), (9, 2047, 3), (10, 2049, 2), (19, 2049, 1), (11, 3000, 2), (12, 3000, 3), (14, 300, 2), (20, 700, 2), (21, 129, 1), (22, 1500, 0)]
SCHEDS = [0, 31, 32]   # the fibers' order: first in first out, and two drawn wave schedules (EMU_SCHED_SEED)


@pytest.mark.parametrize("sched", SCHEDS, ids=lambda s: "sched%d" % s)
@pytest.mark.parametrize("case", SEEDED, ids=lambda c: "seed%d-N%d-len%d" % c)
def test_runs_from_drawn_cluster_states(emu_bin, case, sched):
    """Five launches on one state (services A, B, A, C, B: the third finds the entries and chains the first left), every written array
    against the model after each."""
    run_ok(emu_bin, "seeded", *case, sched=sched)


EDGES = ["error", "packed_below", "clamp", "negzero", "exactk"]


@pytest.mark.parametrize("sched", SCHEDS, ids=lambda s: "sched%d" % s)
@pytest.mark.parametrize("name", EDGES)
def test_fixed_edges(emu_bin, name, sched):
    """error: Ctl.error already set, the launch writes nothing at all. packed_below: svcCount 2^24 - 1 and failure class 254, the last
    values the packed key holds, ranked by their true values. clamp: residuals near 2^62 against a reservation of 1. negzero: the filter
    on with a reservation of 0 / 0 refuses a negative residual and takes a residual of 0. exactk: residuals of exactly k reservations,
    one below, one above."""
    err = run_ok(emu_bin, "edge", name, sched=sched)
    got = reach(err)
    assert got["true_model_differs"] == 0
    if name == "error":
        assert "0 placed, 0 without a node" in err
    if name == "negzero":
        assert got["zero_vs_negative"] > 0
    if name == "clamp":
        assert got["huge_residual"] > 0 and got["tails"] == 0
    if name == "exactk":
        assert got["exact_fit"] > 0 and got["tails"] > 0


def test_a_node_beyond_the_packed_key_gets_capacity_zero(emu_bin):
    """What k_waterfill does with svcCount 2^24 or failure class 255 (259 recorded failures), recorded by name: such a node gets capacity 0
    for the whole run, where the reference only ranks it last — the harness compares the kernel with the model under THAT rule and counts
    how many placements the true ranking would make differently (3 of this case's 5: the tasks end as "no node" instead of landing on the
    two nodes). The kernel must therefore never be handed such a list: build_batch sends a run of such a service to the block resolver
    (tests/test_engine_waterfill.py::test_failure_counts_beyond_the_packed_class pins that on the GPU)."""
    got = reach(run_ok(emu_bin, "edge", "packed_at"))
    assert got["true_model_differs"] == 3


REACH = ["phases", "multi_count_phases", "entries_found", "entries_created", "on_clean", "on_fail_below", "on_fail_at", "on_fail_above", "on_fail_only",
         "on_svc_positive", "holes", "maxrep_cut", "negative_refused", "zero_vs_negative", "resource_refused", "exact_fit", "tails", "none_eligible",
         "lapped_runs", "chain_continued", "list_reused", "tie_across_thread", "tie_across_wave", "huge_residual"]


def test_reach(emu_bin):
    """Across the seeded cases the MODEL's run must have met: phases, phases that walk several distinct task counts, entries found (with
    svcCount > 0; clean; failures below, at and above MAX_FAILURES; failures only) and created, holes, MaxReplicas cut-offs, refusals at a
    negative residual (also of a reservation of 0), residuals that fit exactly, tails without a node, runs without an eligible node, runs
    of several laps, chains picked up from an earlier stretch, entries an earlier launch created, ties by node index across thread and
    wave borders, residuals near 2^62."""
    got = {}
    for c in SEEDED:
        for k, v in reach(run_ok(emu_bin, "seeded", *c)).items():
            got[k] = got.get(k, 0) + v
    print("reach total:", " ".join("%s=%d" % (k, got[k]) for k in REACH))
    for k in REACH:
        assert got[k] > 0, (k, got)
