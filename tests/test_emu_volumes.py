"""CPU: the CSI volume code (swarmkit_amd/csrc/swp_volumes.hpp: vol_check, vol_for_mount, vol_filter_word, vol_choose, vol_reserve,
k_vol_choose, k_vol_topology) and the preassigned pair pass (swp_fitpairs.hpp: k_fit_pairs_vol, and k_fit_pairs for calls without
mounts) run on fibers
(tests/emu/wv_emu.hpp) against the volume model of tests/emu/emu_model.hpp: a per-node, per-mount restatement of the reference's
VolumeSet that keeps usage as (task, node, read-only) and derives the device's {tasks, writers, pin} from it. The model itself is
pinned by the known answers of tests/kat_volumes.py (selftest). No GPU involved; the GPU parity is tests/test_engine_volumes.py and
tests/test_engine_preassigned_mounts.py.

Every "reach" figure asserted below is counted by the MODEL's run (never taken from a kernel's output): a case cannot pass by
reaching nothing."""
import functools
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
BIN = os.path.join(HERE, "_build", "emu_volumes")
CSRC = os.path.join(HERE, "..", "swarmkit_amd", "csrc")


@pytest.fixture(scope="module")
def emu_bin():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    srcs = [os.path.join(EMU, "emu_volumes.cpp"), os.path.join(EMU, "wv_emu.hpp"), os.path.join(EMU, "emu_model.hpp"),
            os.path.join(CSRC, "swp_volumes.hpp"), os.path.join(CSRC, "swp_fitpairs.hpp"), os.path.join(CSRC, "swp_types.hpp")]
    if not os.path.exists(BIN) or any(os.path.getmtime(s) > os.path.getmtime(BIN) for s in srcs):
        tmp = BIN + ".%d.tmp" % os.getpid()   # (xdist workers may build at the same time)
        subprocess.run(["g++", "-O1", "-std=c++17", "-o", tmp, srcs[0]], check=True)
        os.replace(tmp, BIN)
    return BIN


@functools.lru_cache(maxsize=None)
def _run(binary, args):
    r = subprocess.run([binary] + list(args), capture_output=True, text=True, timeout=900)
    return r.returncode, r.stderr


def run_ok(binary, *args):
    rc, err = _run(binary, tuple(str(a) for a in args))
    assert rc == 0, err[-3000:]
    assert "-> OK" in err, err[-3000:]
    return err


def reach(err, label):
    """The figures of the harness's "reach <label>: k=v ..." line."""
    m = re.search(r"^reach %s: ?(.*)$" % re.escape(label), err, re.M)
    assert m, err[-2000:]
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", m.group(1))}


def total(dicts):
    out = {}
    for d in dicts:
        for k, v in d.items():
            out[k] = out.get(k, 0) + v
    return out


# what each mode's committed seeds must reach TOGETHER: every sharing mode with a writing and with a read-only mount, a single-node
# volume in use on the node asked and on another one, a volume whose usages sit on several nodes (pin "many"), a choice that fails at
# mount 0 and one that fails behind a non-empty prefix, a mount refused because of the same task's earlier temporary reservation
VOLUME_REACH = ["none_rw", "none_ro", "readonly_rw", "readonly_ro", "onewriter_rw", "onewriter_ro", "all_rw", "all_ro", "single_here", "single_elsewhere",
                "pin_many", "fail_first", "fail_later", "choice_ok", "refused_by_own"]


def test_model_against_known_answers(emu_bin):
    """The model (and vol_check) against the checkVolume and IsInTopology tables of tests/kat_volumes.py, stated in ids: model and
    kernel cannot share one misreading of the reference."""
    err = run_ok(emu_bin, "selftest")
    assert "9 checkVolume rows, 9 topology rows" in err


FUNCTIONS = [(1, 300), (2, 65), (3, 129), (4, 1000), (5, 64)]   # (seed, nodes): node counts that are not a multiple of 64, one word, many words


@pytest.mark.parametrize("case", FUNCTIONS, ids=lambda c: "seed%d-N%d" % c)
def test_volume_functions(emu_bin, case):
    """k_vol_choose's eleven words for every (mount set, node); vol_filter_word for every (set, word), bit for bit (a bit beyond the last
    node is 0); vol_reserve over a sequence of placements: {tasks, writers, pin} of every volume after each one."""
    run_ok(emu_bin, "functions", *case)


def test_volume_functions_reach(emu_bin):
    got = total(reach(run_ok(emu_bin, "functions", *c), "functions") for c in FUNCTIONS)
    for k in VOLUME_REACH:
        assert got[k] > 0, (k, got)


TOPOLOGY = [(3, 1), (3, 63), (3, 64), (3, 65), (3, 257), (8, 700)]


@pytest.mark.parametrize("case", TOPOLOGY, ids=lambda c: "seed%d-N%d" % c)
def test_topology_bitmaps(emu_bin, case):
    """k_vol_topology over its real grid (workgroup row = volume, two launches with vol0 > 0 for the second) against IsInTopology per
    (node, volume): every word of T, the bits beyond the last node included."""
    run_ok(emu_bin, "topology", *case)


def test_topology_reach(emu_bin):
    """Nodes without a CSIInfo entry of the driver, with one that has no topology, with two of the same plugin; volumes without
    topologies; a wanted segment with id 0 against a missing subdomain; nodes that fit and nodes that do not."""
    got = total(reach(run_ok(emu_bin, "topology", *c), "topology") for c in TOPOLOGY)
    for k in ["no_csi", "no_topology", "plugin_twice", "no_accessible", "zero_vs_missing", "fits", "misses"]:
        assert got[k] > 0, (k, got)


# (seed, segments, pairs of segment 0 (0: as the others), "z": no volume exists)
FITPAIRS = [(1, 1, 0, ""), (2, 255, 0, ""), (3, 256, 0, ""), (4, 257, 300, ""), (5, 3000, 400, ""), (6, 300, 0, "z"), (7, 1, 500, "")]


@pytest.mark.parametrize("case", FITPAIRS, ids=lambda c: "seed%d-seg%d-hot%d%s" % c)
def test_fit_pairs_with_mounts(emu_bin, case):
    """k_fit_pairs_vol (workgroups of 256, one thread per node segment) against a sequential loop over the pairs in segment order: the
    first failing filter of every pair, every attachment row (the chosen prefix on SWP_FIT_NO_VOLUME, VOL_NONE rows otherwise), the
    node rows, generic counts, service counts and host ports after the booking between pairs; the volumes' usage unchanged."""
    run_ok(emu_bin, "fitpairs", *[x for x in case if x != ""])


def test_fit_pairs_reach(emu_bin):
    errs = [run_ok(emu_bin, "fitpairs", *[x for x in c if x != ""]) for c in FITPAIRS]
    got = total(reach(e, "fitpairs") for e in errs)
    for k in VOLUME_REACH:
        assert got[k] > 0, (k, got)
    shapes = [reach(e, "fitpairs shapes") for e in errs]
    for k in ["ff_pass"] + ["ff%d" % f for f in range(9)]:   # every first-fail value -1, 0 .. 8 in at least one case
        assert any(s[k] > 0 for s in shapes), k
    for k in ["clamped", "drained_segments", "uncounted", "port_of_a_pair_in_front", "maxrep_inside"]:
        assert any(s[k] > 0 for s in shapes), k
    novol = shapes[[c[3] for c in FITPAIRS].index("z")]
    assert novol["ff7"] > 0 and novol["ff8"] == 0   # no volume exists: VolumesFilter fails every mount template


# the plain kernel over the same segment counts and hot sizes, and 257 segments of ordinary size: the second workgroup holds one live thread
FITPAIRS_PLAIN = [(c[0], c[1], c[2], "p") for c in FITPAIRS if c[3] == ""] + [(8, 257, 0, "p")]


@pytest.mark.parametrize("case", FITPAIRS_PLAIN, ids=lambda c: "seed%d-seg%d-hot%d%s" % c)
def test_fit_pairs_without_mounts(emu_bin, case):
    """k_fit_pairs — the same segment walk instantiated without mounts, FitArgs alone — against the same sequential loop (no template has
    a mount set: its VolumesFilter and choose lines do nothing): verdicts, node rows, generic counts, service counts and host ports; no
    attachment row is touched."""
    run_ok(emu_bin, "fitpairs", *case)


def test_fit_pairs_without_mounts_reach(emu_bin):
    shapes = [reach(run_ok(emu_bin, "fitpairs", *c), "fitpairs shapes") for c in FITPAIRS_PLAIN]
    for k in ["ff_pass"] + ["ff%d" % f for f in range(7)]:   # every first-fail value -1, 0 .. 6 in at least one case
        assert any(s[k] > 0 for s in shapes), k
    assert all(s["ff7"] == 0 and s["ff8"] == 0 for s in shapes)
    for k in ["clamped", "drained_segments", "uncounted", "port_of_a_pair_in_front", "maxrep_inside"]:
        assert any(s[k] > 0 for s in shapes), k
