"""The streamed tick of task groups without a GPU (include/swp.h swp_schedule_groups_streamed): the rule that says behind which groups
the kernel appends a mark (swarmkit_amd/csrc/swp_rounds.hpp group_pub_step / group_marks), compiled alone into a program of its own
(tests/emu/emu_group_marks.cpp) — once plainly, once under the address and undefined-behaviour sanitizers — and the marks fed through
StreamMarks as the driver feeds them; the new name in the header, the binding and the library.

What must hold is stated here, not read off the code: a mark lies behind group g iff the groups since the previous mark hold at least
`step` tasks or g is the last one; step = the knob, and for a tick of more than 2048 groups at least ceil(total / 2048) (a tick has
no more marks than groups, so only such a tick could fill the ring); marks fall only at group ends, the last one is the total, there
are at most 2048 of them (half the 4096-entry ring); the ranges made of them cover the tick exactly once, every range but the last
holds at least min_tasks tasks and ends at a group boundary.
TEST INFRASTRUCTURE around product source; no product code path uses it."""
import os
import re
import subprocess

import pytest

from swarmkit_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU = os.path.join(HERE, "emu")
CSRC = os.path.join(ROOT, "swarmkit_amd", "csrc")
RING = 4096


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def emu_bin(request):
    out = os.path.join(HERE, "_build", "emu_group_marks_" + request.param)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    srcs = [os.path.join(EMU, "emu_group_marks.cpp"), os.path.join(CSRC, "swp_rounds.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs):
        tmp = out + ".%d.tmp" % os.getpid()   # (xdist workers may build at the same time)
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O1"]
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", tmp, srcs[0]], check=True)
        os.replace(tmp, out)
    return out


def run(emu_bin, *args, env=None):
    base = {k: v for k, v in os.environ.items() if k != "SWP_STREAM_GROUP_TASKS"}
    base.update(env or {})
    r = subprocess.run([emu_bin] + [str(a) for a in args], capture_output=True, text=True, timeout=60, env=base)
    assert r.returncode == 0, (args, r.stdout[-500:], r.stderr[-2000:])
    return r.stdout


def tick(emu_bin, knob, min_tasks, spec):
    lines = run(emu_bin, "tick", knob, min_tasks, *["%dx%d" % ab for ab in spec]).splitlines()
    head = lines[0].split()
    step, total, groups = int(head[1]), int(head[3]), int(head[5])
    marks = [(int(l.split()[1]), int(l.split()[3])) for l in lines if l.startswith("mark ")]
    ranges = [(int(l.split()[1]), int(l.split()[2])) for l in lines if l.startswith("range ")]
    end = [int(x) for x in lines[-1].split()[1:]]
    return dict(step=step, total=total, groups=groups, marks=marks, ranges=ranges, delivered=end[0], top=end[1], taken=end[2], complete=bool(end[3]), bad=bool(end[4]), n_marks=end[5])


def want_marks(sizes, step):
    """The rule, written again from its statement."""
    out, since, end = [], 0, 0
    for g, k in enumerate(sizes):
        since += k
        end += k
        if since >= step or g == len(sizes) - 1:
            out.append((end, g))
            since = 0
    return out


def expand(spec):
    return [b for a, b in spec for _ in range(a)]


CYCLE = [(1, 1), (1, 63), (1, 64), (1, 65), (1, 100)] * 8          # the GPU test's 40 groups
TICKS = [
    # (knob, spec)
    (1, CYCLE),                                                     # step 1: a mark behind every group
    (128, CYCLE),
    (1024, CYCLE),
    (10 ** 6, CYCLE),                                               # a step larger than the total: one mark, at the end
    (1, [(5000, 1)]),                                               # more groups than half the ring: the ring bound cuts the step
    (1, [(3000, 1), (1, 7000), (2500, 1)]),
    (1, [(2049, 3)]),
    (1, [(2048, 3)]),                                               # exactly half the ring: a mark behind every group still fits
    (1024, [(1000, 100)]),                                          # the bench shape
    (1, [(1, 1)]),
]


@pytest.mark.parametrize("min_tasks", [0, 1, 300, 10 ** 7])
@pytest.mark.parametrize("knob,spec", TICKS, ids=lambda v: str(v)[:40])
def test_marks_follow_the_rule_and_the_ranges_cover_the_tick_once(emu_bin, knob, spec, min_tasks):
    sizes = expand(spec)
    total = sum(sizes)
    got = tick(emu_bin, knob, min_tasks, spec)
    step = max(knob, -(-total // (RING // 2))) if len(sizes) > RING // 2 else knob
    assert got["step"] == step and got["total"] == total and got["groups"] == len(sizes)
    assert got["marks"] == want_marks(sizes, step) and got["n_marks"] == len(got["marks"])
    ends = set()
    e = 0
    for k in sizes:
        e += k
        ends.add(e)
    assert all(m in ends for m, _ in got["marks"])                  # only at group ends
    assert got["marks"][-1] == (total, len(sizes) - 1)              # the last mark is the total
    assert len(got["marks"]) <= RING // 2                           # the ring can never wrap inside one launch
    assert all(b > a for (a, _), (b, _) in zip(got["marks"], got["marks"][1:]))
    # through StreamMarks: contiguous, ascending, covering [0, total) once; every range but the last at least min_tasks; ends at marks
    assert got["complete"] and not got["bad"] and got["taken"] == len(got["marks"]) and got["delivered"] == total
    pos = 0
    mark_ends = {m for m, _ in got["marks"]}
    for first, count in got["ranges"]:
        assert first == pos and count > 0
        pos += count
        assert pos in mark_ends
    assert pos == total
    assert all(c >= max(min_tasks, 1) for _, c in got["ranges"][:-1])
    if min_tasks <= 1:
        assert [f + c for f, c in got["ranges"]] == [m for m, _ in got["marks"]]   # every mark is one call
    if min_tasks > total:
        assert got["ranges"] == [(0, total)]
    assert tick(emu_bin, knob, min_tasks, spec) == got              # the same sizes, the same calls


def test_literal_ticks(emu_bin):
    got = tick(emu_bin, 128, 0, CYCLE[:5] * 2)                      # 1, 63, 64, 65, 100, twice
    assert got["marks"] == [(128, 2), (293, 4), (421, 7), (586, 9)]
    assert got["ranges"] == [(0, 128), (128, 165), (293, 128), (421, 165)]
    got = tick(emu_bin, 128, 300, CYCLE[:5] * 2)
    assert got["ranges"] == [(0, 421), (421, 165)]
    got = tick(emu_bin, 1, 0, [(5000, 1)])                          # ceil(5000 / 2048) = 3
    assert got["step"] == 3 and len(got["marks"]) == 1667 and got["marks"][0] == (3, 2) and got["marks"][-1] == (5000, 4999)


def test_the_knob(emu_bin):
    assert run(emu_bin, "knob").strip() == "1024"
    for env, want in [("1", "1"), ("128", "128"), ("8192", "8192"), ("0", "1"), ("-5", "1"), ("x", "1"), ("99999999999", str(0x7FFFFFFF))]:
        assert run(emu_bin, "knob", env={"SWP_STREAM_GROUP_TASKS": env}).strip() == want


def test_header_binding_and_library_name_the_streamed_groups_entry():
    header = open(os.path.join(ROOT, "include", "swp.h")).read()
    declared = set(re.findall(r"\b(swp_[a-z_]+)\s*\(", header))
    L = abi.load_library()
    name = "swp_schedule_groups_streamed"
    assert name in declared and name in abi.EXPORTS and hasattr(L, name)
    assert name in abi.OPTIONAL   # (the host layer's CPU test double has no device pass to stream)
    assert hasattr(abi.Engine, "schedule_groups_streamed")
    assert "have no streamed form" not in header
    assert re.search(r"int swp_schedule_groups_streamed\(swp_engine\*, const swp_task_desc\* groups, const uint32_t\* sizes, uint32_t n_groups,\s*"
                     r"int32_t\* out_node, uint32_t\* out_fail_hist, uint32_t\* out_att,\s*swp_prefix_sink sink, void\* ctx, uint32_t min_tasks\);", header)
