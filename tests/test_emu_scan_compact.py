"""CPU: the COMPACT instance of the scan resolver (swarmkit_amd/csrc/swp_scan.hpp: k_scan_mark, k_scan_union, k_scan_fill_c,
k_scan_lists_c, k_scan<.., .., true>) on fibers: clusters of 5 000 - 9 000 nodes, more than a workgroup's LDS holds, of which 1 .. 4 096
are in any class row of the stretch. The kernels work on that union, the sequential model of tests/emu/emu_model.hpp on ALL nodes:
every output and every mutated array must agree. No GPU involved; the GPU parity is tests/test_engine_scan_compact.py."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
BIN = os.path.join(HERE, "_build", "emu_scan_compact")
CSRC = os.path.join(HERE, "..", "swarmkit_amd", "csrc")


@pytest.fixture(scope="module")
def emu_bin():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    srcs = [os.path.join(EMU, "emu_scan_compact.cpp"), os.path.join(EMU, "wv_emu.hpp"), os.path.join(EMU, "emu_model.hpp"),
            os.path.join(CSRC, "swp_scan.hpp"), os.path.join(CSRC, "swp_resolve6.hpp"), os.path.join(CSRC, "swp_shard.hpp"), os.path.join(CSRC, "swp_types.hpp")]
    if not os.path.exists(BIN) or any(os.path.getmtime(s) > os.path.getmtime(BIN) for s in srcs):
        tmp = BIN + ".%d.tmp" % os.getpid()   # (xdist workers may build at the same time)
        subprocess.run(["g++", "-O1", "-std=c++17", "-o", tmp, srcs[0]], check=True)
        os.replace(tmp, BIN)
    return BIN


# (seed, nodes, tasks, services, block, task order, feature level, eligible nodes, extra)
# feature level 1: heavy services, MaxReplicas, pre-existing exception lists (entries on nodes outside the union among them);
# 2: host ports and RT_UNCOUNTED tasks; 3: generic reservations. Two class rows in eleven are empty: tasks that find no node.
CASES = [
    (1, 5000, 600, 12, 64, 0, 1, 1, ""),          # one eligible node (the last one of the cluster)
    (2, 5003, 900, 20, 64, 0, 2, 9, ""),          # the last node and the first / last bits of words
    (3, 6000, 1200, 30, 64, 2, 2, 700, ""),       # one node per thread; host ports, uncounted tasks, random order
    (4, 7001, 1500, 40, 64, 0, 3, 1024, ""),      # exactly a node per thread; generic reservations
    (5, 8000, 1200, 40, 128, 0, 3, 1025, "g"),    # two per thread, the last thread's second one; matrices in global memory
    (6, 9000, 900, 25, 64, 1, 3, 2500, ""),       # four per thread, service-major
    (7, 8191, 700, 25, 64, 0, 2, 4096, ""),       # the most the kernel takes
    (7, 8191, 700, 25, 64, 0, 2, 4096, "g"),
    (8, 5000, 2000, 6, 64, 0, 1, 300, ""),        # few services on a small pool: every node soon runs every service
    (9, 6500, 1500, 30, 64, 0, 3, 1800, "m"),     # block resolver / compact scan / block resolver in thirds
    (10, 5100, 1200, 20, 64, 2, 2, 600, "mg"),
]
MIX = {"ports": (2, 4, 5, 6, 7, 9), "generic": (4, 5, 6, 9), "maxrep": (2, 3, 4, 5, 6, 7, 9, 10), "uncounted": (2, 4, 5, 6, 9)}   # seeds whose batch must hold such tasks


def run(emu_bin, case, env=None):
    args = [str(x) for x in case[:8]] + ["v"] + list(case[8])
    r = subprocess.run([emu_bin] + args, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "-> OK" in r.stderr
    return r.stderr


@pytest.mark.parametrize("case", CASES, ids=lambda c: "seed%d-N%d-T%d-f%d-Nc%d%s" % (c[0], c[1], c[2], c[6], c[7], c[8]))
def test_compact_scan_source_matches_the_model_over_all_nodes(emu_bin, case):
    err = run(emu_bin, case)
    m = re.search(r"union (\d+) \| placed (\d+) inf (\d+) \| tasks with ports (\d+) generic (\d+) maxrep (\d+) uncounted (\d+)", err)
    union, placed, inf = int(m.group(1)), int(m.group(2)), int(m.group(3))
    if "m" not in case[8]:
        assert union == case[7]   # (a third of the batch need not name every class row)
    assert placed > 0 and inf > 0, "the case must hold tasks that find a node and tasks that find none"
    have = dict(zip(("ports", "generic", "maxrep", "uncounted"), (int(m.group(i)) for i in (4, 5, 6, 7))))
    for what, seeds in MIX.items():
        if case[0] in seeds:
            assert have[what] > 0, "seed %d no longer has tasks with %s" % (case[0], what)


def test_the_probes_arithmetic(emu_bin):
    """The map is ascending, scan_c_of is its inverse, the matrices hold a cell per list entry inside the union and the lists stay as
    they were (the harness checks it on every run and says so): eligible bits at both ends of words, pre-existing lists all over the cluster."""
    err = run(emu_bin, CASES[1])
    assert "union of 9 nodes (asked for 9), map ascending, inverse and matrices agree: OK" in err
    err = run(emu_bin, CASES[6])
    assert "union of 4096 nodes (asked for 4096), map ascending, inverse and matrices agree: OK" in err


@pytest.mark.parametrize("case", [CASES[2], CASES[4], CASES[9]], ids=lambda c: "seed%d-N%d-T%d-f%d-Nc%d%s" % (c[0], c[1], c[2], c[6], c[7], c[8]))
def test_under_random_wave_schedules(emu_bin, case):
    """... under wave orders the first-in-first-out run never produces (EMU_SCHED_SEED, tests/emu/wv_emu.hpp)."""
    run(emu_bin, case, env=dict(os.environ, EMU_SCHED_SEED="31"))
