"""Builds tests/_build/libswpfakefitvol.so: the engine double with swp_fit_pairs (tests/fake_swp.cpp + tests/fake_fit.cpp) plus
tests/fake_fitvol.cpp, which gives it swp_fit_pairs_volumes, linked with the C++ host layer (swarmkit_amd/csrc/swp_sched.cpp): the host
layer then keeps tasks with cluster mounts inside its preassigned runs. tests/test_preassigned_mounts_cpu.py compares it with the plain
double's library (no pair entry at all: the per-task path). SWP_FAKE_SANITIZE=1 builds it under AddressSanitizer + UBSan, as
tests/fakelib.py builds the plain double."""
import ctypes
import os
import subprocess

import fakefit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "_build", "libswpfakefitvol.so")
SRCS = fakefit.SRCS + [os.path.join(ROOT, "tests", "fake_fitvol.cpp")]
DEPS = fakefit.DEPS + [os.path.join(ROOT, "tests", "fake_fitvol.cpp")]


def build():
    san = os.environ.get("SWP_FAKE_SANITIZE") == "1"
    out = OUT.replace(".so", "_san.so") if san else OUT
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in DEPS):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    tmp = "%s.%d.tmp" % (out, os.getpid())   # parallel test workers: build privately, publish atomically
    extra = ["-O0", "-fsanitize=address,undefined,float-cast-overflow", "-fno-omit-frame-pointer"] if san else []
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fPIC", "-shared"] + extra + ["-o", tmp] + SRCS, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("libswpfakefitvol.so build failed:\n" + r.stdout + r.stderr)
    os.replace(tmp, out)
    return out


def calls(lib_path):
    """(swp_fit_pairs calls, swp_fit_pairs_volumes calls) the library has seen so far, refused ones included."""
    L = ctypes.CDLL(lib_path)
    L.swp_fake_fit_calls.restype = ctypes.c_uint64
    L.swp_fake_fitvol_calls.restype = ctypes.c_uint64
    return L.swp_fake_fit_calls(), L.swp_fake_fitvol_calls()
