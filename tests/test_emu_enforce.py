"""CPU: k_enforce_generic (swarmkit_amd/csrc/swp_enforce.hpp — the enforcer sweep for nodes whose tasks hold AssignedGenericResources,
one wave per node, the node's list in the lanes) runs on fibers (tests/emu/wv_emu.hpp) against the sequential model of
tests/emu/emu_enforce.cpp, written from the reference's loop body, HasResource and ConsumeNodeResources on plain vectors. No GPU
involved; the GPU parity is tests/test_engine_enforce_generic.py.

Every "reach" figure asserted below is counted by the MODEL's run (never taken from the kernel's output): a case cannot pass by
reaching nothing."""
import functools
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
BIN = os.path.join(HERE, "_build", "emu_enforce")
CSRC = os.path.join(HERE, "..", "swarmkit_amd", "csrc")


@pytest.fixture(scope="module")
def emu_bin():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    srcs = [os.path.join(EMU, "emu_enforce.cpp"), os.path.join(EMU, "wv_emu.hpp"), os.path.join(CSRC, "swp_enforce.hpp"), os.path.join(CSRC, "swp_types.hpp")]
    if not os.path.exists(BIN) or any(os.path.getmtime(s) > os.path.getmtime(BIN) for s in srcs):
        tmp = BIN + ".%d.tmp" % os.getpid()   # (xdist workers may build at the same time)
        subprocess.run(["g++", "-O1", "-std=c++17", "-o", tmp, srcs[0]], check=True)
        os.replace(tmp, BIN)
    return BIN


@functools.lru_cache(maxsize=None)
def _run(binary, args):
    r = subprocess.run([binary] + list(args), capture_output=True, text=True, timeout=300)
    return r.returncode, r.stderr


def run_ok(binary, *args):
    rc, err = _run(binary, tuple(str(a) for a in args))
    assert rc == 0, err[-3000:]
    assert "-> OK" in err, err[-3000:]
    return err


def reach(err):
    m = re.search(r"^reach sweep: ?(.*)$", err, re.M)
    assert m, err[-2000:]
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", m.group(1))}


# (seed, nodes): one wave, a workgroup that is not full, exactly one workgroup, several
SWEEPS = [(1, 1), (2, 3), (3, 4), (4, 5), (5, 64), (6, 150), (7, 150), (8, 257)]


@pytest.mark.parametrize("case", SWEEPS, ids=lambda c: "seed%d-N%d" % c)
def test_sweep(emu_bin, case):
    """Every verdict byte of every node against the model (a byte the kernel never wrote shows as 0xAA), nothing written behind the last
    task; of the lists longer than a wave, what is left of them in the work copy; the shorter ones never written there."""
    run_ok(emu_bin, "sweep", *case)


def test_sweep_reach(emu_bin):
    got = {}
    for c in SWEEPS:
        for k, v in reach(run_ok(emu_bin, "sweep", *c)).items():
            got[k] = got.get(k, 0) + v
    # break-loop taken; a task behind a break that the walk would have rejected; a type mismatch under one kind; one assignment meeting two
    # Discrete entries of its kind (a kind listed twice); two assignments of one kind subtracting from one entry; a Discrete entry reaching
    # exactly 0; a task with assignments on a list of more than 64 entries, and one decided by an entry behind the 64th
    for k in ["break_loop", "behind_break_rejected", "type_mismatch", "kind_twice", "two_assignments", "exact_zero", "long_list", "decided_past_64",
              "claimed", "plain_rejected", "skipped", "nil_or_empty"]:
        assert got[k] > 0, (k, got)
