"""The host rule of the block resolver's ring rounds (swarmkit_amd/csrc/swp_rounds.hpp: r6_ring, r6_ring_block, r6_ring_stream_every,
RoundRules::ring / block) without a GPU: tests/emu/emu_rounds_ring.cpp includes the header alone and prints what it gives for scripted
inputs. The expected values are LITERALS worked out from the rule's text: the ring is on where the long lists are, the batch has no
cluster mounts, the engine is single, the node set has more than 128 half-words (more than 64 node words: more than 4 096 nodes), the
stretch has more tasks left than a flat block holds, and SWP_R6_BLOCK is not set; SWP_R6_RING=0 never, =1 wherever the kernel allows it.
TEST INFRASTRUCTURE around product source; no product code path uses it."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
CSRC = os.path.join(HERE, "..", "swarmkit_amd", "csrc")
BIN = os.path.join(HERE, "_build", "emu_rounds_ring")
KNOBS = ("SWP_DBG", "SWP_R6_BLOCK", "SWP_R6_TASKROWS", "SWP_R6_RUNS", "SWP_R6_COMPACT", "SWP_R6_COMPACT_FUSED", "SWP_SCAN", "SWP_R6_TWINS", "SWP_R6_LEVELS", "SWP_R6_RING")


@pytest.fixture(scope="module")
def emu_bin():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    srcs = [os.path.join(EMU, "emu_rounds_ring.cpp"), os.path.join(CSRC, "swp_rounds.hpp")]
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


def ring(emu_bin, ext_on, mounts, single, n_words, left, flat, env=None):
    return int(run(emu_bin, "ring", ext_on, mounts, single, n_words, left, flat, env=env))


def test_the_headline_and_each_gate(emu_bin):
    """cfg3 100k x 10k: 157 node words, a flat block of 1 408. Each condition switched off alone switches the ring off."""
    assert ring(emu_bin, 1, 0, 1, 157, 100000, 1408) == 1
    assert ring(emu_bin, 0, 0, 1, 157, 100000, 1408) == 0   # no long lists: a batch of runs, a shrunk block (churn rounds, compact index)
    assert ring(emu_bin, 1, 1, 1, 157, 100000, 1408) == 0   # cluster mounts
    assert ring(emu_bin, 1, 0, 0, 157, 100000, 1408) == 0   # the shards
    assert ring(emu_bin, 1, 0, 1, 64, 100000, 1408) == 0    # 128 half-words: not MORE than a ring list holds
    assert ring(emu_bin, 1, 0, 1, 65, 100000, 1408) == 1
    assert ring(emu_bin, 1, 0, 1, 157, 1408, 1408) == 0     # what is left fits a flat block
    assert ring(emu_bin, 1, 0, 1, 157, 1409, 1408) == 1
    assert ring(emu_bin, 1, 0, 1, 157, 100000, 1408, env={"SWP_R6_BLOCK": "1408"}) == 0   # a forced block stays flat
    assert ring(emu_bin, 1, 0, 1, 625, 200000, 1344) == 1   # cfg4 200k x 40k
    assert ring(emu_bin, 1, 0, 1, 1563, 1000000, 1216) == 1  # 1M x 100k


@pytest.mark.parametrize("n_nodes,tasks,block", [(2304, 7000, 1408), (4096, 3000, 1408), (4096, 3000, 1400), (2304, 7000, 256), (200, 2000, 64)],
                         ids=["levels-2304", "ahead-heads-window-4096", "window-4096-1400", "levels-2304-256", "stream-200"])
def test_the_existing_gpu_tests_shapes_keep_flat_blocks(emu_bin, n_nodes, tasks, block):
    """test_engine_levels (2 304 nodes), _ahead, _heads and _window (4 096 nodes), with and without their SWP_R6_BLOCK: the node sets
    have at most 128 half-words, so their round counts — never fewer than ceil(T / block) — stand."""
    words = (n_nodes + 63) // 64
    assert ring(emu_bin, 1, 0, 1, words, tasks, block) == 0
    assert ring(emu_bin, 1, 0, 1, words, tasks, block, env={"SWP_R6_BLOCK": str(block)}) == 0


def test_the_knob(emu_bin):
    assert ring(emu_bin, 1, 0, 1, 157, 100000, 1408, env={"SWP_R6_RING": "0"}) == 0
    # 1: wherever the kernel allows it — a small node set, a stretch that would fit flat, a forced block ...
    assert ring(emu_bin, 1, 0, 1, 64, 100, 1408, env={"SWP_R6_RING": "1"}) == 1
    assert ring(emu_bin, 1, 0, 1, 2, 1200, 1088, env={"SWP_R6_RING": "1", "SWP_R6_BLOCK": "1088"}) == 1
    # ... but not where it does not: no long lists, cluster mounts, the shards
    assert ring(emu_bin, 0, 0, 1, 157, 100000, 1408, env={"SWP_R6_RING": "1"}) == 0
    assert ring(emu_bin, 1, 1, 1, 157, 100000, 1408, env={"SWP_R6_RING": "1"}) == 0
    assert ring(emu_bin, 1, 0, 0, 157, 100000, 1408, env={"SWP_R6_RING": "1"}) == 0


def test_ring_block_and_stream_cadence(emu_bin):
    assert int(run(emu_bin, "block", 2048, 2816)) == 2816                                   # the rule's block
    assert int(run(emu_bin, "block", 1088, 2816, env={"SWP_R6_BLOCK": "1088"})) == 1088     # SWP_R6_BLOCK with SWP_R6_RING=1
    assert int(run(emu_bin, "block", 1100, 2816, env={"SWP_R6_BLOCK": "1100"})) == 1088     # whole groups
    assert int(run(emu_bin, "block", 10, 2816, env={"SWP_R6_BLOCK": "10"})) == 64
    assert int(run(emu_bin, "block", 2048, 2048, env={"SWP_R6_BLOCK": "2048"})) == 2048
    # publishes every 8 rounds of 1 408 tasks = every 4 rounds of 2 816; never less than every round
    assert int(run(emu_bin, "every", 8, 1408, 2816)) == 4
    assert int(run(emu_bin, "every", 1, 1408, 2816)) == 1
    assert int(run(emu_bin, "every", 8, 1088, 1088)) == 8
    assert int(run(emu_bin, "every", 3, 1408, 2816)) == 1


def test_a_stretch_ends_on_flat_rounds(emu_bin):
    """100 000 tasks, flat 1 408, ring 2 816: ring rounds while more than a flat block is left, then the flat block with its long
    lists; the first chunk is the pace's sixteen rounds, the second 1.05 x (54 944 / 2 816) + 4 = 24."""
    out = run(emu_bin, "drive", 0, 100000, 1408, 2816, 157, 1, 45056, 16, 98560, 35, 99990, 36).split("\n")
    assert out[0] == "1 2816 1 16"
    assert out[1] == "1 2816 1 24"
    assert out[2] == "1 2816 1 4"      # 1 440 left: more than a flat block
    assert out[3] == "0 1408 1 4"      # 10 left
    # a stretch that fits a flat block, a small node set, a batch of runs: paced with the flat block, as ever
    assert run(emu_bin, "drive", 0, 1408, 1408, 2816, 157, 1).split("\n")[0] == "0 1408 1 7"
    assert run(emu_bin, "drive", 0, 7000, 1408, 2816, 36, 1).split("\n")[0] == "0 1408 1 16"
    assert run(emu_bin, "drive", 0, 100000, 768, 2816, 157, 0).split("\n")[0] == "0 768 0 16"
    # rounds that decide a fraction of their block: the pace shrinks it and the ring goes; below the flat block the long lists go too
    out = run(emu_bin, "drive", 0, 100000, 1408, 2816, 157, 1, 1600, 16).split("\n")
    assert out[1] == "0 256 0 64"
    out = run(emu_bin, "drive", 0, 100000, 1408, 2816, 157, 1, 16000, 16).split("\n")   # 1 000 a round: 2 x 1 000 rounded up to 64s = 2 048 > flat
    assert out[1] == "0 1408 1 64"      # ... a flat block with its long lists, as without a ring
