"""Builds tests/_build/libswpfakeenforce.so: the plain engine double (tests/fake_swp.cpp) plus tests/fake_enforce.cpp, which gives it
swp_enforce_generic, linked with the C++ host layer (swarmkit_amd/csrc/swp_sched.cpp): the host layer then sends a sweep whose tasks hold
AssignedGenericResources through that one entry. tests/test_enforce_generic_cpu.py compares it with the plain double's library (no such
entry: swp_enforce, then the host layer's own walk). SWP_FAKE_SANITIZE=1 builds it under AddressSanitizer + UBSan, as tests/fakelib.py
builds the plain double."""
import ctypes
import os
import subprocess

import fakelib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "_build", "libswpfakeenforce.so")
SRCS = fakelib.SRCS + [os.path.join(ROOT, "tests", "fake_enforce.cpp")]
DEPS = fakelib.DEPS + [os.path.join(ROOT, "tests", "fake_enforce.cpp")]


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
        raise RuntimeError("libswpfakeenforce.so build failed:\n" + r.stdout + r.stderr)
    os.replace(tmp, out)
    return out


def calls(lib_path):
    """swp_enforce_generic calls the library has seen so far, refused ones included."""
    L = ctypes.CDLL(lib_path)
    L.swp_fake_enforce_generic_calls.restype = ctypes.c_uint64
    return L.swp_fake_enforce_generic_calls()
