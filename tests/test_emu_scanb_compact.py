"""CPU: the COMPACT BATCHED instance of the scan resolver (swarmkit_amd/csrc/swp_scan.hpp: k_scan_mark, k_scan_union, k_scan_fill_c,
k_scan_lists_c, k_scanb<.., true>, scan_lds_bc) on fibers: clusters of 5 000 - 9 000 nodes, more than a workgroup's LDS holds, of which
1 .. 2 100 are in any class row of the stretch. The kernels work on that union, the sequential model of tests/emu/emu_model.hpp on ALL
nodes: every output and every mutated array must agree. The harness restates the launcher's rule and says which instance ran. No GPU
involved; the GPU parity is tests/test_engine_scanb_compact.py."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
BIN = os.path.join(HERE, "_build", "emu_scanb_compact")
CSRC = os.path.join(HERE, "..", "swarmkit_amd", "csrc")
BUDGET = 160 * 1024 - 512


@pytest.fixture(scope="module")
def emu_bin():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    srcs = [os.path.join(EMU, "emu_scanb_compact.cpp"), os.path.join(EMU, "wv_emu.hpp"), os.path.join(EMU, "emu_model.hpp"),
            os.path.join(CSRC, "swp_scan.hpp"), os.path.join(CSRC, "swp_resolve6.hpp"), os.path.join(CSRC, "swp_shard.hpp"), os.path.join(CSRC, "swp_types.hpp")]
    if not os.path.exists(BIN) or any(os.path.getmtime(s) > os.path.getmtime(BIN) for s in srcs):
        tmp = BIN + ".%d.tmp" % os.getpid()   # (xdist workers may build at the same time)
        subprocess.run(["g++", "-O1", "-std=c++17", "-o", tmp, srcs[0]], check=True)
        os.replace(tmp, BIN)
    return BIN


# (seed, nodes, tasks, services, block, task order, feature level, eligible nodes, extra)
# feature level 1: heavy services, MaxReplicas, pre-existing exception lists (entries on nodes outside the union among them). The harness
# adds: the last service asks for an empty class row (four rows are empty: tasks that find no node), from three services on service 1
# is RT_UNCOUNTED, from four on service 2 has a replica limit of 2. extra: n = no descriptor ids (nothing is skipped), m = block resolver /
# compact batched scan / block resolver in thirds, k<len> = stretches of len, 2 len + 1, 4 len + 3 ... tasks, a probe each.
CASES = [
    (1, 5000, 600, 3, 64, 0, 1, 1, ""),             # one eligible node (the last one of the cluster)
    (2, 5003, 900, 4, 64, 0, 1, 9, ""),             # the last node and the first / last bits of words
    (3, 6000, 1200, 6, 64, 0, 1, 256, ""),          # exactly one node a thread
    (4, 7001, 1500, 5, 64, 0, 1, 257, ""),          # the last thread's second node: NQ 2
    (5, 8000, 1500, 4, 64, 2, 1, 700, "k3"),        # NQ 4; random order; a stretch of 3 tasks, then 7, 15, ... (none a multiple of 256)
    (6, 9000, 1800, 4, 64, 1, 1, 1500, ""),         # NQ 8, service-major
    (7, 8191, 1500, 4, 64, 0, 1, 2100, ""),         # NQ 16
    (8, 6500, 1200, 6, 64, 0, 1, 2100, ""),         # six services on 2 100 nodes: the rows do NOT fit, k_scan<.., .., true> runs
    (9, 5100, 1000, 3, 64, 0, 1, 300, "n"),         # no descriptor ids: nothing skipped
    (10, 6500, 1500, 5, 64, 0, 1, 600, "m"),        # block resolver / compact batched scan / block resolver in thirds
    (11, 5000, 2000, 2, 64, 0, 1, 300, "k100"),     # a saturated pool: two services, stretches of 100, 201, 403, ... tasks
]
NQ = {1: 1, 2: 1, 3: 1, 4: 2, 5: 4, 6: 8, 7: 16, 9: 2, 10: 4, 11: 2}          # seed -> nodes a thread of the instance that must run
NO_FIT = (8,)
SKIPS = (2, 4, 6, 7, 11)                                                     # seeds whose run must answer tasks without a look
MIX = {"maxrep": (2, 3, 4, 5, 6, 7, 10), "uncounted": (1, 2, 3, 4, 5, 6, 7, 10), "heavy": (2, 4, 5, 6, 11), "outside": (3, 4, 5, 6, 7, 10)}
LINE = re.compile(r"union (\d+) nq (\d+) \| placed (\d+) inf (\d+) skipped (\d+) \| k_scanb launches (\d+) k_scan launches (\d+) shortest stretch (\d+) \| "
                  r"tasks with maxrep (\d+) uncounted (\d+) heavy (\d+), list entries outside the union (\d+)")
ROWS_OK = "class rows over the compact space equal the gather of the original rows through the map"


def ident(c):
    return "seed%d-N%d-T%d-S%d-Nc%d%s" % (c[0], c[1], c[2], c[3], c[7], c[8])


def run(emu_bin, case, env=None):
    args = [str(x) for x in case[:8]] + ["v"] + ([case[8]] if case[8] else [])
    r = subprocess.run([emu_bin] + args, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "-> OK" in r.stderr
    return r.stderr


def lds_bc(n_c, n_svc, n_sc):
    """scan_lds_bc restated: node rows, the two matrices, the class rows over the union; three sets of argmins, the queue, a window's
    records and ids, the table of descriptors."""
    return ((n_c * 24 + 15) & ~15) + 2 * n_svc * n_c * 4 + n_sc * ((n_c + 63) // 64) * 8 + 3 * 4 * 8 + (256 // 64) * 8 + 16 + 256 * 64 + 256 * 4 + 1024 * 4


@pytest.mark.parametrize("case", CASES, ids=ident)
def test_compact_batched_scan_source_matches_the_model_over_all_nodes(emu_bin, case):
    err = run(emu_bin, case)
    print(err)
    m = LINE.search(err)
    union, nq, placed, inf, skipped, by_b, by_one, shortest = (int(m.group(i)) for i in range(1, 9))
    assert union == case[7]
    assert placed > 0 and inf > 0, "the case must hold tasks that find a node and tasks that find none"
    assert ROWS_OK in err and ROWS_OK + " (%d stretches): OK" % (by_b + by_one) in err
    f = re.search(r"footprint: scan_lds_bc\((\d+), (\d+), (\d+)\) = (\d+) bytes of (\d+) -> (fits|does not fit)", err)
    assert int(f.group(4)) == lds_bc(union, case[3], int(f.group(3))) and int(f.group(5)) == BUDGET
    if case[0] in NO_FIT:
        assert int(f.group(4)) > BUDGET and f.group(6) == "does not fit" and "(k_scan) runs" in err
        assert by_b == 0 and by_one > 0 and skipped == 0
    else:
        assert int(f.group(4)) <= BUDGET and f.group(6) == "fits"
        assert by_b > 0 and by_one == 0 and nq == NQ[case[0]]
    if case[0] in SKIPS:
        assert skipped > 0, "seed %d no longer answers a task without a look" % case[0]
    if "n" in case[8]:
        assert skipped == 0
    if case[8] == "k3":
        assert shortest == 3
    assert case[2] % 256 != 0 or case[8].startswith("k")
    have = dict(zip(("maxrep", "uncounted", "heavy", "outside"), (int(m.group(i)) for i in (9, 10, 11, 12))))
    for what, seeds in MIX.items():
        if case[0] in seeds:
            assert have[what] > 0, "seed %d no longer has %s" % (case[0], what)


@pytest.mark.parametrize("case", [CASES[3], CASES[4], CASES[9]], ids=ident)
def test_under_random_wave_schedules(emu_bin, case):
    """... under wave orders the first-in-first-out run never produces (EMU_SCHED_SEED, tests/emu/wv_emu.hpp)."""
    run(emu_bin, case, env=dict(os.environ, EMU_SCHED_SEED="31"))
