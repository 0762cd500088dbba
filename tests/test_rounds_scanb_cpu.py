"""The single engine's scan loop over a CONDITIONAL hand-over (a cluster beyond the scan resolver's node count), without a GPU:
tests/emu/emu_rounds_scanb.cpp restates run_stretch's loop around swarmkit_amd/csrc/swp_rounds.hpp with a scripted device. What is new
with the batched instance's compact form: `fast` is a property of the STRETCH there (ScanHandover::looks' stretch_fast), the words are
read behind such a stretch, `again` follows with the next stretch behind a probe of its own, and a refusal there is a refusal like any
other, back-off included.

The expected lines are literals worked out by hand from the rules' text: 20 000 tasks, rounds of one task each. The first chunk is
min(16, 20000 / 256 + 1) = 16 rounds, and sixteen poor rounds are due (>= 8). The first stretch is [16, 16 + 2048). Behind it the next
one is twice as long: [2064, 2064 + 4096); too wide, the one shorter try is an eighth, [2064, 2064 + 512); refused, the hold is
2064 + 2048 = 4112 and doubles to 4096, and while it holds no probe is due."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
CSRC = os.path.join(HERE, "..", "swarmkit_amd", "csrc")
BIN = os.path.join(HERE, "_build", "emu_rounds_scanb")


@pytest.fixture(scope="module")
def emu_bin():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    srcs = [os.path.join(EMU, "emu_rounds_scanb.cpp"), os.path.join(CSRC, "swp_rounds.hpp")]
    if not os.path.exists(BIN) or any(os.path.getmtime(s) > os.path.getmtime(BIN) for s in srcs):
        tmp = BIN + ".%d.tmp" % os.getpid()   # (xdist workers may build at the same time)
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", tmp, srcs[0]], check=True)
        os.replace(tmp, BIN)
    return BIN


def run(emu_bin, *args):
    r = subprocess.run([emu_bin] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def test_a_batched_stretch_mostly_skipped_is_followed_at_once_and_a_refusal_there_holds(emu_bin):
    """Three quarters of the first stretch are answered without a look; the next stretch's union (5 000 nodes) is too wide."""
    out = run(emu_bin, 20000, 1024, 750, 600, 5000)
    assert out[:6] == ["rounds 16 pos 16 held 0 scan 1",
                       "probe 16 2064 union 600",
                       "stretch 16 2064 batched 1 looks 1 again 1 chunk 4",
                       "probe 2064 6160 union 5000",          # no round in between: its own probe first
                       "probe 2064 2576 union 5000",
                       "refused at 2064 hold_until 4112 hold 4096 chunk 64"]
    assert all(l.endswith("held 1 scan 0") for l in out[6:-1]) and len(out) > 8   # the rounds carry on, no probe while the hold lasts
    assert out[-1] == "probes 3 refusals 1 scanned 2048"


def test_a_stretch_of_the_one_task_instance_is_not_looked_behind(emu_bin):
    """A union too large for the batched form: nobody reads the words, four probing rounds follow every stretch."""
    out = run(emu_bin, 20000, 1024, 750, 2000)
    assert out[:4] == ["rounds 16 pos 16 held 0 scan 1", "probe 16 2064 union 2000", "stretch 16 2064 batched 0 looks 0 again 0 chunk 4",
                       "rounds 4 pos 2068 held 0 scan 1"]
    assert not any(" looks 1" in l or " again 1" in l for l in out)


def test_a_batched_stretch_with_few_skipped_goes_back_to_the_rounds(emu_bin):
    """A quarter skipped: the words are read, `again` says no; the last stretch (it ends the batch) is not looked behind."""
    out = run(emu_bin, 20000, 1024, 250, 600)
    assert out[2] == "stretch 16 2064 batched 1 looks 1 again 0 chunk 4" and out[3] == "rounds 4 pos 2068 held 0 scan 1"
    assert out[-2] == "stretch 14364 20000 batched 1 looks 0 again 0 chunk 4"
    assert not any(" again 1" in l for l in out)
