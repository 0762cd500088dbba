"""CPU: k_spread_cut (swarmkit_amd/csrc/swp_scan_spread.hpp: where a compact spread segment whose class rows' union is too wide is cut
into pieces) on fibers against the sequential bitset model of tests/emu/emu_spread_cut.cpp — the status, the task an own row is
reported for, the piece list word for word, the number of counts made, nothing written behind the list. The limit L is a parameter
of the kernel, so the cases use small ones. Each case also asserts that the event it is named for happened.
No GPU involved; the GPU parity against the oracle is tests/test_engine_oneoff_spread_cut.py."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
BIN = os.path.join(HERE, "_build", "emu_spread_cut")
CSRC = os.path.join(HERE, "..", "swarmkit_amd", "csrc")


@pytest.fixture(scope="module")
def emu_bin():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    srcs = [os.path.join(EMU, "emu_spread_cut.cpp"), os.path.join(EMU, "wv_emu.hpp"),
            os.path.join(CSRC, "swp_scan_spread.hpp"), os.path.join(CSRC, "swp_scan.hpp"), os.path.join(CSRC, "swp_resolve6.hpp"),
            os.path.join(CSRC, "swp_shard.hpp"), os.path.join(CSRC, "swp_types.hpp")]
    if not os.path.exists(BIN) or any(os.path.getmtime(s) > os.path.getmtime(BIN) for s in srcs):
        tmp = BIN + ".%d.tmp" % os.getpid()   # (xdist workers may build at the same time)
        subprocess.run(["g++", "-O1", "-std=c++17", "-o", tmp, srcs[0]], check=True)
        os.replace(tmp, BIN)
    return BIN


OK, OWN_ROW, FULL = 0, 1, 2


def _run(emu_bin, name, where="", env=None):
    r = subprocess.run([emu_bin, name] + ([where] if where else []), capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "-> OK" in r.stderr
    m = re.search(r"status (\d+) task (\d+) \| pieces (\d+) \| cuts at a plain task (\d+) \| cuts at a task with preferences (\d+) \| rows counted again (\d+) \| "
                  r"rode along (\d+) \| counts (\d+) \| at the limit (\d+) \| one over (\d+)", r.stderr)
    ev = dict(zip(("status", "task", "pieces", "cut_plain", "cut_pref", "again", "rode", "counts", "at_limit", "one_over"), (int(x) for x in m.groups())))
    ev["list"] = [tuple(int(x) for x in p) for p in re.findall(r"\((\d+),(\d+),(\d+)\)", r.stderr.split("list:")[1].split("\n")[0])]
    ev["words"] = int(re.search(r"words (\d+)", r.stderr).group(1))
    ev["n_sc"] = int(re.search(r"n_sc (\d+)", r.stderr).group(1))
    return ev


# the small cases: the whole list is stated here as well (the harness compares the kernel's words with the model's)
@pytest.mark.parametrize("where", ["", "g"], ids=["lds", "global"])
@pytest.mark.parametrize("name,status,task,pieces", [
    ("nocut", OK, 0, [(0, 6, 1)]),
    ("plain_cut", OK, 0, [(0, 3, 1), (3, 2, 0), (5, 3, 1)]),          # a plain task that does not fit: spread, plain, spread
    ("pref_cut", OK, 0, [(0, 3, 1), (3, 3, 1)]),                      # a task with preferences that does not fit: nothing in between
    ("exact_L", OK, 0, [(0, 5, 1)]),
    ("L_plus_1", OK, 0, [(0, 2, 1), (2, 2, 1), (4, 1, 0)]),
    ("row_again", OK, 0, [(0, 1, 1), (1, 1, 1), (2, 2, 1), (4, 1, 0), (5, 1, 1)]),
    ("own_row", OWN_ROW, 3, [(0, 3, 1)]),
    ("own_row_first", OWN_ROW, 3, []),
    ("plain_wide_row", OK, 0, [(0, 2, 1), (2, 2, 0), (4, 1, 1)]),
    ("full", FULL, 0, [(0, 1, 1), (1, 1, 1), (2, 1, 1)]),
    ("full_exact", OK, 0, [(0, 1, 1), (1, 1, 1), (2, 1, 1), (3, 1, 1)]),
    ("boundary", OK, 0, [(0, 1024, 1), (1024, 1023, 1), (2047, 2, 0), (2049, 451, 1)]),
    ("boundary_j0", OK, 0, [(37, 1024, 1), (1061, 1023, 1), (2084, 2, 0), (2086, 451, 1)]),
    ("nsc1", OK, 0, [(0, 76, 1)]),
])
def test_cut_kernel_source_matches_the_rule(emu_bin, name, status, task, pieces, where):
    ev = _run(emu_bin, name, where)
    assert (ev["status"], ev["task"]) == (status, task)
    assert ev["list"] == pieces and ev["pieces"] == len(pieces)
    cuts = ev["cut_plain"] + ev["cut_pref"]
    if name in ("nocut", "exact_L", "nsc1"):
        assert cuts == 0
    if name == "plain_cut":
        assert ev["cut_plain"] == 1 and ev["cut_pref"] == 0
    if name == "pref_cut":
        assert ev["cut_plain"] == 0 and ev["cut_pref"] == 1
    if name == "exact_L":
        assert ev["at_limit"] == 1 and ev["one_over"] == 0
    if name == "L_plus_1":
        assert ev["one_over"] >= 1 and cuts >= 1
    if name == "row_again":
        assert ev["again"] >= 1 and cuts >= 1
    if name == "plain_wide_row":
        assert ev["cut_plain"] == 1
    if name.startswith("boundary"):   # 2 500 tasks, 7 counts: the tasks whose row the piece holds ride along unseen
        assert ev["rode"] == 2493 and ev["counts"] == 7 and ev["cut_plain"] == 1 and ev["cut_pref"] == 1
    if name == "nsc1":
        assert ev["n_sc"] == 1 and ev["counts"] == 1


# random rows and segments: n_sc 65 and 300, 4 097 and 9 000 nodes (65 and 141 words: no multiple of the 1 024 threads), and 70 000
# nodes (1 094 words: a thread takes more than one)
@pytest.mark.parametrize("where", ["", "g"], ids=["lds", "global"])
@pytest.mark.parametrize("name,n_sc,words", [("nsc65", 65, 65), ("nsc300", 300, 141), ("n9000", 40, 141), ("n70000", 30, 1094)])
def test_random_segments(emu_bin, name, n_sc, words, where):
    ev = _run(emu_bin, name, where)
    assert ev["status"] == OK and (ev["n_sc"], ev["words"]) == (n_sc, words)
    assert ev["cut_plain"] > 0 and ev["cut_pref"] > 0 and ev["again"] > 0 and ev["rode"] > 0
    assert ev["pieces"] >= ev["cut_plain"] + ev["cut_pref"] + 1


@pytest.mark.parametrize("sched", [31, 77])
@pytest.mark.parametrize("name", ["boundary_j0", "nsc300", "n70000"])
def test_under_random_wave_schedules(emu_bin, name, sched):
    """... under wave orders the first-in-first-out run never produces (EMU_SCHED_SEED, tests/emu/wv_emu.hpp)."""
    ev = _run(emu_bin, name, env=dict(os.environ, EMU_SCHED_SEED=str(sched)))
    assert ev["status"] == OK and ev["cut_plain"] > 0 and ev["cut_pref"] > 0
