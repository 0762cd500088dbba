"""Builds tests/_build/libswpfakefit.so: the plain engine double (tests/fake_swp.cpp) plus tests/fake_fit.cpp, which gives it the
swp_fit_pairs the host layer's preassigned path batches through, linked with the C++ host layer (swarmkit_amd/csrc/swp_sched.cpp).
tests/test_preassigned_batch_cpu.py compares it with the plain double's library (libswpfake.so, no swp_fit_pairs: the per-task path)."""
import ctypes
import os
import subprocess

import fakelib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "_build", "libswpfakefit.so")
SRCS = fakelib.SRCS + [os.path.join(ROOT, "tests", "fake_fit.cpp")]
DEPS = fakelib.DEPS + [os.path.join(ROOT, "tests", "fake_fit.cpp")]


def build():
    if os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(d) for d in DEPS):
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    tmp = "%s.%d.tmp" % (OUT, os.getpid())   # parallel test workers: build privately, publish atomically
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fPIC", "-shared", "-o", tmp] + SRCS, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("libswpfakefit.so build failed:\n" + r.stdout + r.stderr)
    os.replace(tmp, OUT)
    return OUT


def fit_calls(lib_path):
    """swp_fit_pairs calls the library has seen so far (refused ones included)."""
    fn = ctypes.CDLL(lib_path).swp_fake_fit_calls
    fn.restype = ctypes.c_uint64
    return fn()
