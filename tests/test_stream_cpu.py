"""The streamed run without a GPU (include/swp.h swp_batch_run_streamed): the arithmetic that turns the marks of the device's
publishes into deliveries to the caller's sink (swarmkit_amd/csrc/swp_rounds.hpp StreamMarks), compiled alone into a program of its own
(tests/emu/emu_stream.cpp) — once plainly, once under the address and undefined-behaviour sanitizers — and fed scripted mark sequences;
the new names in the header, the binding and the library; k_publish in the shipped objects.

What a sequence of deliveries must satisfy is stated here, not read off the code: the ranges are contiguous, ascending and cover [0, T)
exactly once when the last mark is T; every range but the last holds at least max(min_tasks, 1) tasks; a range ends at a mark; with
min_tasks = 0 every mark that moved is one delivery; the same marks give the same deliveries.
TEST INFRASTRUCTURE around product source; no product code path uses it."""
import os
import re
import subprocess
import sys

import pytest

from swarmkit_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU = os.path.join(HERE, "emu")
CSRC = os.path.join(ROOT, "swarmkit_amd", "csrc")
NEW_NAMES = ["swp_batch_run_streamed", "swp_schedule_batch_streamed"]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def emu_bin(request):
    out = os.path.join(HERE, "_build", "emu_stream_" + request.param)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    srcs = [os.path.join(EMU, "emu_stream.cpp"), os.path.join(CSRC, "swp_rounds.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs):
        tmp = out + ".%d.tmp" % os.getpid()   # (xdist workers may build at the same time)
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O1"]
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", tmp, srcs[0]], check=True)
        os.replace(tmp, out)
    return out


def run(emu_bin, *args, env=None):
    base = {k: v for k, v in os.environ.items() if k != "SWP_STREAM_EVERY"}
    base.update(env or {})
    r = subprocess.run([emu_bin] + [str(a) for a in args], capture_output=True, text=True, timeout=60, env=base)
    assert r.returncode == 0, (args, r.stdout, r.stderr)
    return r.stdout


def deliveries(emu_bin, T, min_tasks, marks):
    lines = run(emu_bin, "marks", T, min_tasks, *marks).splitlines()
    end = lines[-1].split()
    assert end[0] == "end"
    delivered, top, taken, complete, bad = (int(x) for x in end[1:])
    return [tuple(int(x) for x in l.split()) for l in lines[:-1]], dict(delivered=delivered, top=top, taken=taken, complete=bool(complete), bad=bool(bad))


def check_contract(T, min_tasks, marks, got, end):
    """The header's contract for marks that end at T."""
    assert end["taken"] == len(marks) and not end["bad"]
    pos = 0
    for first, count in got:
        assert first == pos and count > 0
        pos += count
        assert pos in marks   # a range ends where a publish ended
    assert pos == T == end["delivered"] and end["complete"]
    for first, count in got[:-1]:
        assert count >= max(min_tasks, 1)


SCRIPTS = [
    # (T, marks): every one ends at T
    (1, [1]),
    (2000, [2000]),                                                   # one mark at T
    (2000, [64, 64, 64, 130, 130, 512, 512, 1999, 2000, 2000]),       # repeats: publishes that found no progress
    (2000, [0, 0, 64, 128, 192, 256, 320, 1000, 1001, 1002, 2000]),   # marks before anything was decided
    (300, list(range(1, 301))),                                       # a mark per task
    (65, [63, 64, 65]),
]


@pytest.mark.parametrize("min_tasks", [0, 1, 100, 5000])
@pytest.mark.parametrize("T,marks", SCRIPTS)
def test_deliveries_cover_the_batch_once(emu_bin, T, marks, min_tasks):
    got, end = deliveries(emu_bin, T, min_tasks, marks)
    check_contract(T, min_tasks, marks, got, end)
    again, _ = deliveries(emu_bin, T, min_tasks, marks)
    assert again == got                                               # the same marks, the same calls
    if min_tasks <= 1:                                                # one delivery per mark that moved
        moved = sorted(set(m for m in marks if m > 0))
        assert [f + c for f, c in got] == moved
    if min_tasks > T:                                                 # nothing is due before the end: one range
        assert got == [(0, T)]


def test_literal_sequences(emu_bin):
    marks = [64, 64, 64, 130, 130, 512, 512, 1999, 2000, 2000]
    assert deliveries(emu_bin, 2000, 0, marks)[0] == [(0, 64), (64, 66), (130, 382), (512, 1487), (1999, 1)]
    assert deliveries(emu_bin, 2000, 100, marks)[0] == [(0, 130), (130, 382), (512, 1487), (1999, 1)]   # 64 < 100 waits for the next mark; the last range may be short
    assert deliveries(emu_bin, 2000, 400, marks)[0] == [(0, 512), (512, 1487), (1999, 1)]


def test_no_marks_and_marks_that_stop_short(emu_bin):
    got, end = deliveries(emu_bin, 500, 0, [])
    assert got == [] and not end["complete"] and end["delivered"] == 0            # (the engine reports that: nothing was published)
    got, end = deliveries(emu_bin, 500, 100, [64, 450])
    assert got == [(0, 450)] and not end["complete"] and end["top"] == 450
    got, end = deliveries(emu_bin, 500, 100, [450, 460])                           # 10 tasks pending below min_tasks, and not the end
    assert got == [(0, 450)] and end["delivered"] == 450 and end["top"] == 460 and not end["complete"]
    got, end = deliveries(emu_bin, 0, 0, [])                                       # a batch without tasks: no call, nothing missing
    assert got == [] and end["complete"]


def test_marks_the_device_cannot_have_written(emu_bin):
    """Beyond T, or behind an earlier mark: the ring does not hold what k_publish wrote — nothing of it is delivered."""
    got, end = deliveries(emu_bin, 500, 0, [100, 501])
    assert got == [(0, 100)] and end["bad"] and not end["complete"]
    got, end = deliveries(emu_bin, 500, 0, [100, 99, 500])
    assert got[0] == (0, 100) and end["bad"] and not end["complete"]


def test_the_ring_is_drained_before_it_wraps(emu_bin):
    out = run(emu_bin, "ring", 4100).split()
    outstanding, ring = int(out[-2]), int(out[-1])
    room = [int(x) for x in out[:-2]]
    assert ring == 4096 and outstanding == 4100
    assert room[:ring - 1] == [1] * (ring - 1) and not any(room[ring - 1:])       # the driver waits for the stream before the 4096th


def test_stream_every_knob(emu_bin):
    assert run(emu_bin, "every").strip() == "8"
    for env, want in [("4", "4"), ("32", "32"), ("0", "1"), ("-3", "1"), ("100000", "4096"), ("x", "1")]:
        assert run(emu_bin, "every", env={"SWP_STREAM_EVERY": env}).strip() == want


def test_header_binding_and_library_name_the_streamed_entries():
    header = open(os.path.join(ROOT, "include", "swp.h")).read()
    declared = set(re.findall(r"\b(swp_[a-z_]+)\s*\(", header))
    L = abi.load_library()
    for name in NEW_NAMES:
        assert name in declared and name in abi.EXPORTS and hasattr(L, name), name
        assert name in abi.OPTIONAL   # (the host layer's CPU test double has no device pass to stream)
    assert re.search(r"typedef\s+int\s*\(\*swp_prefix_sink\)\(void\* ctx, uint32_t first, uint32_t count, const int32_t\* nodes\);", header)
    codes = dict(re.findall(r"\b(SWP_E[A-Z]+)\s*=\s*(-\d+)", header))
    assert int(codes["SWP_ECANCELLED"]) == abi.SWP_ECANCELLED == min(int(v) for v in codes.values())   # behind the last code there was
    assert L.swp_strerror(abi.SWP_ECANCELLED) not in (None, b"unknown error")
    assert hasattr(abi.Engine, "schedule_batch_streamed") and hasattr(abi.Batch, "run_streamed")


def test_k_publish_ships_and_passes_the_kernel_checks():
    abi.build_library()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_kernels.py"), "--verbose"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    line = [l for l in r.stdout.splitlines() if " k_publish " in l]
    assert len(line) == 1, r.stdout
    assert " scratch    0 " in line[0] and "vgpr-spill 0" in line[0] and "sgpr-spill 0" in line[0], line[0]
