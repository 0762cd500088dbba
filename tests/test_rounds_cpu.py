"""The host rules of the block resolver's round drivers (swarmkit_amd/csrc/swp_rounds.hpp: knobs, row mode, the block that fits the
commit kernel's LDS, the pace) without a GPU: tests/emu/emu_rounds.cpp includes the header alone and prints what it gives for scripted
inputs. batch_run_impl, swp_shard_run and swp_shard_run_rank all take their chunk and block from it; between ranks a different chunk on
one rank means collectives that no longer line up, so the numbers are pinned here.

The expected values are LITERALS: recorded once from the expressions the three drivers carried themselves before the header existed
(the first chunk, the recent / chunk / block update of the shard drivers, the inline block update of the single engine), compiled as a
separate program — not computed from the code under test. Three of them can be checked by hand: block 768 at 100 tasks a round -> 256
(2 x 100 rounded up to 64s); block 256 at 400 a round -> 512 (400 > 0.4 x 256: the next size up); 0.5 a round -> 128 (the floor).

The single engine's own rules (the knobs it used to read itself, runs and window, the compact switch, the scan hand-over, a whole
stretch driven by scripted words: the tests from test_single_engine_knobs on) are pinned the same way: their literals were recorded from
the expressions batch_run_impl, its run_blocks lambda and r6_args_for carried inline before the header took them — the getenv tests, the
switch's update, the hand-over with its backwards goto, copied into a stand-alone program with the launches replaced by prints and the
read-backs by scripted words, compiled once and run on the command lines used here.
TEST INFRASTRUCTURE around product source; no product code path uses it."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
CSRC = os.path.join(HERE, "..", "swarmkit_amd", "csrc")
BIN = os.path.join(HERE, "_build", "emu_rounds")
KNOBS = ("SWP_DBG", "SWP_R6_BLOCK", "SWP_R6_TASKROWS", "SWP_R6_RUNS", "SWP_R6_COMPACT", "SWP_R6_COMPACT_FUSED", "SWP_SCAN", "SWP_R6_TWINS")


@pytest.fixture(scope="module")
def emu_bin():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    srcs = [os.path.join(EMU, "emu_rounds.cpp"), os.path.join(CSRC, "swp_rounds.hpp")]
    if not os.path.exists(BIN) or any(os.path.getmtime(s) > os.path.getmtime(BIN) for s in srcs):
        tmp = BIN + ".%d.tmp" % os.getpid()   # (xdist workers may build at the same time)
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", tmp, srcs[0]], check=True)
        os.replace(tmp, BIN)
    return BIN


def run(emu_bin, *args, env=None):
    base = {k: v for k, v in os.environ.items() if k not in KNOBS}
    base.update(env or {})
    r = subprocess.run([emu_bin] + [str(a) for a in args], capture_output=True, text=True, timeout=60, env=base)
    assert r.returncode == 0, (args, r.stderr)
    return r.stdout


def pairs(out):
    return [tuple(int(x) for x in line.split()) for line in out.splitlines()]


def test_first_chunk(emu_bin):
    """A short stretch does not pay for empty rounds: min(16, n / 256 rounded up + 1)."""
    ns = [1, 255, 256, 257, 1500, 3584, 3840, 3841, 4096, 200000]
    assert [int(x) for x in run(emu_bin, "first", *ns).split()] == [2, 2, 2, 3, 7, 15, 16, 16, 16, 16]


# (block now, tasks per round in the last stretch) -> the next block, with 100 000 tasks left; the same for a largest block of 768 and 1024
# except where the largest block itself is the answer. 0.4 x 128 = 51.2, 0.4 x 256 = 102.4, 0.4 x 768 = 307.2: both sides of each.
BLOCK_RULE = [
    (128, 0.5, 128), (128, 50, 128), (128, 52, 256), (128, 100, 256), (128, 400, 256),
    (256, 0.5, 128), (256, 52, 128), (256, 100, 256), (256, 103, 512), (256, 308, 512), (256, 400, 512),
    (768, 0.5, 128), (768, 52, 128), (768, 100, 256), (768, 103, 256), (768, 307.2, 640),
]


@pytest.mark.parametrize("largest", [768, 1024])
def test_block_follows_the_pace(emu_bin, largest):
    for cur, recent, want in BLOCK_RULE:
        assert pairs(run(emu_bin, "step", 100000, recent, cur, largest, 0)) == [(64, want)], (cur, recent)   # (a small block: look again after 64 rounds)
    # rounds that fill the largest block keep it, and the chunk is what the rest needs
    assert pairs(run(emu_bin, "step", 100000, 308, 768, largest, 0)) == [(344, largest)]
    assert pairs(run(emu_bin, "step", 100000, 400, 768, largest, 0)) == [(266, largest)]


def test_chunk(emu_bin):
    assert pairs(run(emu_bin, "step", 1000, 100, 768, 768, 0)) == [(14, 256)]        # 1000 / 100 x 1.05 + 4
    assert pairs(run(emu_bin, "step", 1000, 0.5, 768, 768, 0)) == [(64, 128)]        # a pace below one task a round counts as one: 1054, but the block is small
    assert pairs(run(emu_bin, "step", 1000, 0.5, 768, 768, 1)) == [(1054, 768)]      # the block forced: no such cap
    assert pairs(run(emu_bin, "step", 1000000, 400, 768, 768, 0)) == [(2629, 768)]
    assert pairs(run(emu_bin, "step", 10000000, 400, 768, 768, 0)) == [(4096, 768)]  # never more than 4096 rounds without a look
    assert pairs(run(emu_bin, "step", 1000000, 10, 768, 768, 1)) == [(4096, 768)]
    assert pairs(run(emu_bin, "step", 1000000, 10, 768, 768, 0)) == [(64, 128)]


WORDS = [300, 7, 340, 12, 900, 16, 1500, 20]   # (position, rounds that found work) read after each chunk of a batch of 1500 tasks


def test_pace_of_a_run(emu_bin):
    """What the shard drivers do with the words of a run: fast rounds, a poor stretch (8 tasks a round: the smallest block, a look every
    64 rounds at most), rounds that fill the small block (the next size up), the end (nothing moves once the batch is decided)."""
    assert pairs(run(emu_bin, "pace", 1500, 768, 0, *WORDS)) == [(7, 768), (33, 128), (64, 128), (8, 256), (4, 256)]


def test_forced_block_never_moves(emu_bin):
    assert pairs(run(emu_bin, "pace", 1500, 64, 1, *WORDS)) == [(7, 64), (33, 64), (156, 64), (8, 64), (4, 64)]   # 156: no cap of 64 rounds either


def test_single_engine_use(emu_bin):
    """batch_run_impl observes first (the hand-over to the scan resolver sits in between) and replans then: the blocks its inline update
    gave. That update also ran after the LAST chunk, into a value nothing read (512 in both runs here); the shared rule leaves the block
    alone there — so the comparison is over the values that were used, and the last entry is the shared rule's."""
    assert pairs(run(emu_bin, "single", 0, 1500, 768, 0, *WORDS)) == [(7, 768), (33, 128), (64, 128), (8, 256), (4, 256)]
    # a stretch that does not start at task 0 (a batch with runs of identical tasks in between), the largest block the kernel takes
    got = pairs(run(emu_bin, "single", 1000, 4000, 1024, 0, 1600, 4, 1650, 9, 1700, 73, 2900, 76, 4000, 80))
    assert got == [(13, 1024), (20, 320), (64, 128), (64, 128), (6, 256), (4, 256)]


def test_fit_block(emu_bin):
    """Down in steps of 64 tasks while the commit kernel's LDS (here base + per x block bytes against 160 KiB - 512) does not hold the
    block; 64 is the floor whatever the size says (the caller refuses then); a block of 64 or less is never touched."""
    assert run(emu_bin, "fit", 768, 100000, 100).strip() == "768 704 640 576 -> 576"
    assert run(emu_bin, "fit", 1000, 90000, 100).strip() == "1000 960 896 832 768 704 -> 704"
    assert run(emu_bin, "fit", 768, 200000, 100).strip() == "768 704 640 576 512 448 384 320 256 192 128 -> 64"
    assert run(emu_bin, "fit", 768, 0, 100).strip() == "768 -> 768"
    assert run(emu_bin, "fit", 64, 200000, 100).strip() == "-> 64"
    assert run(emu_bin, "fit", 33, 200000, 100).strip() == "-> 33"


@pytest.mark.parametrize("env,classes_ok,n,want", [
    (None, 1, 128, 0), (None, 1, 129, 1), (None, 0, 5, 1),      # unset: task rows when the classes overflowed or there are many
    ("0", 1, 128, 0), ("0", 1, 129, 0), ("0", 0, 5, 0),       # the knob wins, either way
    ("1", 1, 128, 1), ("1", 1, 129, 1), ("1", 0, 5, 1),
    ("7", 1, 5, 1),
])
def test_task_rows(emu_bin, env, classes_ok, n, want):
    out = run(emu_bin, "knobs", classes_ok, n, env=None if env is None else {"SWP_R6_TASKROWS": env}).split()
    assert int(out[3]) == (-1 if env is None else int(env != "0")) and int(out[4]) == want


def test_knobs(emu_bin):
    """Read on every call; the block within [1, the kernel's largest]; "forced" means the variable is there, whatever it says."""
    assert run(emu_bin, "knobs", 1, 0).split()[:3] == ["0", "0", "768"]
    assert run(emu_bin, "knobs", 1, 0, env={"SWP_R6_BLOCK": "5000", "SWP_DBG": "48"}).split()[:3] == ["48", "1", "1024"]
    assert run(emu_bin, "knobs", 1, 0, env={"SWP_R6_BLOCK": "0"}).split()[:3] == ["0", "1", "1"]
    assert run(emu_bin, "knobs", 1, 0, env={"SWP_R6_BLOCK": "7"}).split()[:3] == ["0", "1", "7"]


# ---- the single engine's own rules: the knobs it used to read itself, runs and window, the compact switch, the scan hand-over --------
# (where the literals below come from: the module docstring. Not computed from the header under test.)
NEW_KNOBS = ("SWP_R6_RUNS", "SWP_R6_COMPACT", "SWP_R6_COMPACT_FUSED", "SWP_SCAN", "SWP_R6_TWINS")


@pytest.mark.parametrize("env,want", [
    ({}, "-1 -1 1 1 1"),                                    # unset: the batch and the rounds decide; fused, scan and twins on
    ({k: "0" for k in NEW_KNOBS}, "0 0 0 0 0"),
    ({k: "1" for k in NEW_KNOBS}, "1 1 1 1 1"),
    ({k: "abc" for k in NEW_KNOBS}, "0 0 0 0 0"),           # not a number reads as 0
    ({"SWP_R6_COMPACT": "2"}, "-1 1 1 1 1"),                # any non-zero value pins the index on
    ({"SWP_SCAN": "1"}, "-1 -1 1 1 1"),                     # (still on)
])
def test_single_engine_knobs(emu_bin, env, want):
    """runs compact fused scan twins, behind the five fields the shard drivers share (those unchanged by the new variables)."""
    out = run(emu_bin, "knobs", 1, 0, env=env).split()
    assert out[:5] == ["0", "0", "768", "-1", "0"] and " ".join(out[5:]) == want


@pytest.mark.parametrize("T,in_runs,env,want", [
    (1000, 500, {}, "0 0 1408"),                            # exactly half the tasks in runs: an ordinary batch
    (1000, 501, {}, "1 32 768"),                            # one more: whole proposals in LDS, blocks of 768 at most
    (1001, 500, {}, "0 0 1408"),
    (1001, 501, {}, "1 32 768"),
    (1000, 0, {"SWP_R6_RUNS": "1"}, "1 32 768"),            # the knob forces either
    (1000, 1000, {"SWP_R6_RUNS": "0"}, "0 0 1408"),
    (1000, 1000, {"SWP_R6_BLOCK": "1000"}, "1 32 1000"),    # a forced block is not cut to 768
    (1000, 0, {"SWP_R6_BLOCK": "1000"}, "0 0 1000"),
    (1000, 1000, {"SWP_R6_BLOCK": "500"}, "1 32 500"),
    (1000, 1000, {"SWP_R6_BLOCK": "5000"}, "1 32 1408"),    # (within the kernel's largest block)
])
def test_runs_and_window(emu_bin, T, in_runs, env, want):
    assert run(emu_bin, "runs", T, in_runs, env=env).strip() == want


ON = (4, 10, 128, 2, 0, 4)   # (used, recent, block, exh, crounds, stops) of a chunk that switches the index on: every condition just met or well met


@pytest.mark.parametrize("allowed,hint,env,chunks,want,ever", [
    (1, 0, {}, [(3, 10, 128, 2, 0, 4), ON], ["0 0", "0 0", "1 2"], 0),                           # used 3 / 4
    (1, 0, {}, [(5, 10, 128, 2, 0, 5), ON], ["0 0", "0 0", "1 2"], 0),                           # 2 x exh = 4 against used 5 / 4
    (1, 0, {}, [(4, 51.3, 128, 2, 0, 18), (4, 51.1, 128, 2, 0, 18)], ["0 0", "0 0", "1 2"], 0),  # recent either side of 0.4 x 128 = 51.2
    (1, 0, {}, [(4, 12, 128, 2, 0, 3), (4, 12, 128, 2, 0, 4)], ["0 0", "0 0", "1 2"], 0),        # stops x 12 = 36 / 48 against 12 x 4
    # on; three rounds without an index are no verdict; a chunk with one keeps it; four rounds without one switch it off
    (1, 0, {}, [ON, (3, 10, 128, 0, 0, 0), (4, 10, 128, 0, 1, 0), (4, 10, 128, 0, 0, 0)], ["0 0", "1 2", "1 2", "1 2", "0 0"], 1),
    (1, 0, {}, [ON, (4, 10, 128, 0, 0, 0)], ["0 0", "1 2", "0 0"], 0),                           # on and off again without one indexed round: never in use
    (1, 0, {}, [ON, (4, 10, 128, 2, 3, 4), (4, 10, 128, 0, 0, 0), ON], ["0 0", "1 2", "1 2", "0 0", "1 2"], 1),   # on, off, on: `ever` stays
    (1, 0, {"SWP_R6_COMPACT": "1"}, [(4, 10, 128, 0, 0, 0), (4, 10, 128, 0, 1, 0)], ["1 2", "1 2", "1 2"], 1),   # pinned: never off
    (1, 1, {"SWP_R6_COMPACT": "0"}, [ON, ON], ["0 0", "0 0", "0 0"], 0),                         # never on, whatever the hint says
    (1, 1, {}, [(4, 10, 128, 0, 1, 0)], ["1 2", "1 2"], 1),                                      # the engine's hint: on from the first round
    (0, 1, {}, [ON], ["0 0", "0 0"], 0),                                                         # not allowed (LDS, volumes): neither hint ...
    (0, 0, {"SWP_R6_COMPACT": "1"}, [ON], ["0 0", "0 0"], 0),                                    # ... nor knob
    (1, 1, {"SWP_R6_COMPACT_FUSED": "0"}, [(4, 10, 128, 0, 1, 0)], ["1 1", "1 1"], 1),           # the index by a launch of its own
])
def test_compact_switch(emu_bin, allowed, hint, env, chunks, want, ever):
    """"on compact" at the start and after each chunk; `ever` is what the engine keeps as the next batch's hint."""
    out = run(emu_bin, "compact", allowed, hint, *[x for c in chunks for x in c], env=env).splitlines()
    assert out == want + ["ever %d" % ever]


def test_scan_due(emu_bin):
    """Four poor rounds (two behind a scan stretch) where the batched scan runs, eight (four) where it does not; poor is fewer than 8
    tasks a round; nothing is handed over with fewer than 64 tasks left."""
    due = lambda out: [int(line.split()[1]) for line in out.splitlines() if line.startswith("due")]
    fast = run(emu_bin, "scan", 1, 1, *"due 3 1.0 1000 due 4 1.0 1000 due 4 7.9 1000 due 4 8.0 1000 due 4 1.0 63 due 4 1.0 64 stretch 0 100000 "
               "due 1 1.0 1000 due 2 1.0 1000 rounds due 3 1.0 1000 due 4 1.0 1000".split())
    assert due(fast) == [0, 1, 1, 0, 0, 1, 0, 1, 0, 1] and "scan 0 2048 2 4096" in fast
    slow = run(emu_bin, "scan", 1, 0, *"due 7 1.0 1000 due 8 1.0 1000 due 8 7.9 1000 due 8 8.0 1000 due 8 1.0 63 due 8 1.0 64 stretch 500 1000 "
               "due 3 1.0 1000 due 4 1.0 1000 rounds due 7 1.0 1000 due 8 1.0 1000".split())
    assert due(slow) == [0, 1, 1, 0, 0, 1, 0, 1, 0, 1] and "scan 500 1000 4 4096" in slow   # (the stretch ends at `end`; four probing rounds)
    assert run(emu_bin, "scan", 0, 1, *"due 100 1.0 1000 cap 1000 1.0 cap 5 1.0".split()).splitlines() == ["due 0", "cap 1000", "cap 5", "scanned 0"]   # SWP_SCAN=0, volumes, wide keys


def test_scan_stretch_length(emu_bin):
    out = run(emu_bin, "scan", 1, 1, *(["stretch", 0, 10000000] * 11)).splitlines()
    lens = [2048 << i for i in range(10)] + [1 << 20]   # 2048, 4096, ... 1 048 576, and no further
    assert out == ["scan 0 %d 2 %d" % (n, min(2 * n, 1 << 20)) for n in lens] + ["scanned 3143680"]


def test_scan_chunk_cap(emu_bin):
    args = "cap 1000 15.9 cap 1000 16 cap 1000 63.9 cap 1000 64 cap 5 1.0".split()
    assert run(emu_bin, "scan", 1, 1, *args).splitlines() == ["cap 8", "cap 16", "cap 16", "cap 256", "cap 5", "scanned 0"]
    assert run(emu_bin, "scan", 1, 0, *args).splitlines() == ["cap 16", "cap 48", "cap 48", "cap 256", "cap 5", "scanned 0"]


def test_scan_again(emu_bin):
    """Another stretch directly behind one of which at least half went without a look (2 x 1023 < 2048; 2 x (3071 - 1023) = 4096), never
    behind one that reached the end."""
    out = run(emu_bin, "scan", 1, 1, *"stretch 0 10000 again 0 2048 10000 1023 stretch 2048 10000 again 2048 6144 10000 3071 stretch 6144 10000 "
              "again 6144 10000 10000 6927".split()).splitlines()
    assert out == ["scan 0 2048 2 4096", "again 0", "scan 2048 6144 2 8192", "again 1", "scan 6144 10000 2 16384", "again 0", "scanned 10000"]
    assert run(emu_bin, "scan", 1, 1, *"stretch 0 2048 again 0 2048 2048 2048".split()).splitlines() == ["scan 0 2048 2 4096", "again 0", "scanned 2048"]


# start end largest forced runs allowed hint scan_ok scan_fast report node_local, then (pos rounds cuts crounds reseats skipped) per read-back
DRIVE = {
    # no hand-over: the pace alone; the longer lists only while the block is the largest
    "plain": ({}, "0 1500 768 0 0 1 0 0 0 0 0  300 7 0 0 9 0  340 12 1 0 20 0  900 16 1 0 30 0  1500 20 1 0 40 0",
              ["rounds 7 768 0 on", "rounds 33 128 0 off", "rounds 64 128 0 off", "rounds 8 256 0 off", "end 1500 ever 0 scanned 0 words 4"]),
    # sixteen poor rounds -> a stretch, mostly answered without a look -> another directly behind it (twice as long) -> two probing rounds
    # with block and ext as they were (no replan) -> good rounds: back to the pace
    "scan_again_back": ({}, "0 20000 768 0 0 1 0 1 1 0 1  40 16 2 0 5 0  2088 16 2 0 5 2000  6184 16 2 0 5 2100  7000 18 2 0 9 2100  20000 40 2 0 30 2100",
                        ["rounds 16 768 0 on", "scan 40 2088", "scan 2088 6184", "rounds 2 768 0 on", "rounds 37 768 0 on", "end 20000 ever 0 scanned 6144 words 5"]),
    # the symptom switches the index on (with the small block the pace picks), a chunk without an indexed round off again
    "compact_on_off": ({}, "0 5000 768 0 0 1 0 0 0 0 0  160 16 16 0 40 0  800 80 70 64 200 0  3000 100 75 64 230 0  5000 110 75 64 240 0",
                       ["rounds 16 768 0 on", "rounds 64 128 2 off", "rounds 64 128 2 off", "rounds 23 256 0 off", "end 5000 ever 1 scanned 0 words 4"]),
    # a stretch that starts at task 1000; the one-task-a-barrier scan: thirteen poor rounds, four probes, no look behind a stretch
    "offset_slow_scan": ({}, "1000 4000 1024 0 0 1 0 1 0 0 0  1030 13 0 0 3 0  3090 17 0 0 4 0",
                         ["rounds 13 1024 0 on", "scan 1030 3078", "rounds 4 1024 0 on", "scan 3090 4000", "end 4000 ever 0 scanned 2958 words 2"]),
    # a stretch that reaches the end: the words behind it are read for the report only (three read-backs against two)
    "scan_to_end_report": ({}, "0 3000 768 0 0 1 0 1 1 1 1  50 13 0 0 3 0  2098 13 0 0 3 2048  3000 13 0 0 3 2950",
                           ["rounds 13 768 0 on", "scan 50 2098", "scan 2098 3000", "end 3000 ever 0 scanned 2950 words 3"]),
    "scan_to_end_no_report": ({}, "0 3000 768 0 0 1 0 1 1 0 1  50 13 0 0 3 0  2098 13 0 0 3 2048",
                              ["rounds 13 768 0 on", "scan 50 2098", "scan 2098 3000", "end 3000 ever 0 scanned 2950 words 2"]),
    # a batch of runs with the block forced and the index pinned, not fused: nothing moves, no longer lists
    "runs_forced_pinned": ({"SWP_R6_COMPACT": "1", "SWP_R6_COMPACT_FUSED": "0"}, "0 1500 512 1 1 1 0 0 0 0 0  300 7 0 7 9 0  340 12 1 12 20 0  1500 20 1 12 40 0",
                           ["rounds 7 512 1 off", "rounds 33 512 1 off", "rounds 156 512 1 off", "end 1500 ever 1 scanned 0 words 3"]),
    # 2 x 1023 < 2048: not again; chunk caps of the hand-over (6 from the pace, then 8); poor rounds with 50 tasks left: no hand-over
    "few_left_not_again": ({}, "0 2200 768 0 0 1 0 1 1 0 1  30 10 0 0 3 0  2078 10 0 0 3 1023  2140 12 0 0 3 1023  2150 16 0 0 3 1023  2200 20 0 0 3 1023",
                           ["rounds 10 768 0 on", "scan 30 2078", "rounds 2 768 0 on", "rounds 6 128 0 off", "rounds 8 128 0 off", "end 2200 ever 0 scanned 2048 words 5"]),
    # the previous batch's hint, switched off by the chunk that also hands over (the switch is fed before the hand-over is decided)
    "hint_then_off_then_scan": ({}, "0 9000 768 0 0 1 1 1 0 0 1  64 16 16 0 30 0  2200 24 20 0 31 0  9000 60 20 0 40 0",
                                ["rounds 16 768 2 on", "scan 64 2112", "rounds 4 768 0 on", "rounds 16 128 0 off", "end 9000 ever 0 scanned 2048 words 3"]),
}


@pytest.mark.parametrize("name", sorted(DRIVE))
def test_drive(emu_bin, name):
    """A whole stretch as batch_run_impl drives it, the device's words scripted: the sequence of launches ("rounds chunk block compact
    ext", "scan j0 j1") and the number of read-backs."""
    env, args, want = DRIVE[name]
    assert run(emu_bin, "drive", *args.split(), env=env).splitlines() == want
