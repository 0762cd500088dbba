#!/usr/bin/env python3
"""Is a kernel's gfx950 code in two builds of an object byte for byte the same? The objects' fat binaries are unbundled (as
tools/check_kernels.py does it), the kernel's bytes in .text and its 64-byte kernel descriptor in .rodata are cut out by their symbols
and compared (the descriptor without its offset to the code). A kernel added next to it moves addresses, not these bytes: the code of
one kernel is position independent.

usage: python tools/cmp_kernel.py <object A> <object B> <kernel name, e.g. k_groups2>      exit code 1 when they differ"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_kernels import LLVM, demangle_short, device_elf   # noqa: E402


def sections(elf):
    out = subprocess.run([f"{LLVM}/llvm-readelf", "-S", "-W", elf], capture_output=True, text=True, check=True).stdout
    secs = {}
    for m in re.finditer(r"\[\s*(\d+)\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", out):
        secs[int(m.group(1))] = (m.group(2), int(m.group(3), 16), int(m.group(4), 16), int(m.group(5), 16))
    return secs


def symbol_bytes(elf, kernel):
    """-> {symbol kind: bytes} for the kernel's function and its descriptor (<name>.kd)"""
    secs = sections(elf)
    data = open(elf, "rb").read()
    out = subprocess.run([f"{LLVM}/llvm-readelf", "-s", "-W", elf], capture_output=True, text=True, check=True).stdout
    got = {}
    for line in out.splitlines():
        f = line.split()
        if len(f) < 8 or not f[6].isdigit():
            continue
        name = f[7]
        kind = "descriptor" if name.endswith(".kd") else "code"
        if demangle_short(name[:-3] if kind == "descriptor" else name) != kernel or f[3] not in ("FUNC", "OBJECT"):
            continue
        addr, size = int(f[1], 16), int(f[2])
        _, sec_addr, sec_off, _ = secs[int(f[6])]
        got[kind] = data[sec_off + addr - sec_addr: sec_off + addr - sec_addr + size]
        if kind == "descriptor":   # (bytes 16-23: the offset from the descriptor to the code — layout, not the kernel)
            got[kind] = got[kind][:16] + bytes(8) + got[kind][24:]
    return got


def main():
    a, b, kernel = sys.argv[1:4]
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        ga, gb = symbol_bytes(device_elf(a, ta), kernel), symbol_bytes(device_elf(b, tb), kernel)
    same = True
    for kind in ("code", "descriptor"):
        if kind not in ga or kind not in gb:
            print(f"cmp_kernel: {kernel}: no {kind} symbol in one of the objects")
            return 1
        eq = ga[kind] == gb[kind]
        same &= eq
        print(f"cmp_kernel: {kernel} {kind}: {len(ga[kind])} vs {len(gb[kind])} bytes, {'identical' if eq else 'DIFFERENT'}")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
