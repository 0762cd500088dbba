"""The host rules of the block resolver's round drivers (swarmkit_amd/csrc/swp_rounds.hpp: knobs, row mode, the block that fits the
commit kernel's LDS, the pace) without a GPU: tests/emu/emu_rounds.cpp includes the header alone and prints what it gives for scripted
inputs. batch_run_impl, swp_shard_run and swp_shard_run_rank all take their chunk and block from it; between ranks a different chunk on
one rank means collectives that no longer line up, so the numbers are pinned here.

The expected values are LITERALS: recorded once from the expressions the three drivers carried themselves before the header existed
(the first chunk, the recent / chunk / block update of the shard drivers, the inline block update of the single engine), compiled as a
separate program — not computed from the code under test. Three of them can be checked by hand: block 768 at 100 tasks a round -> 256
(2 x 100 rounded up to 64s); block 256 at 400 a round -> 512 (400 > 0.4 x 256: the next size up); 0.5 a round -> 128 (the floor).
TEST INFRASTRUCTURE around product source; no product code path uses it."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
CSRC = os.path.join(HERE, "..", "swarmkit_amd", "csrc")
BIN = os.path.join(HERE, "_build", "emu_rounds")
KNOBS = ("SWP_DBG", "SWP_R6_BLOCK", "SWP_R6_TASKROWS")


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
