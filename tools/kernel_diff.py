#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of the library, instruction by instruction.

usage: kernel_diff.py OLD.so NEW.so

Extracts every code object of both (kernel_census.code_objects), disassembles each kernel symbol
and compares the instruction text (addresses dropped; branch targets are relative to the symbol).
Prints the counts and every kernel that is missing, added or different; exit status 1 if any is.
A host-side refactor must leave every kernel identical.
"""
import re
import subprocess
import sys
import tempfile

from kernel_census import LLVM, code_objects


def kernels(lib):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        # keyed by translation unit too: a template instance can be emitted in several of them
        for tu, co in enumerate(code_objects(lib, tmp)):
            syms = subprocess.run([f"{LLVM}/llvm-objdump", "-t", co], check=True, capture_output=True, text=True).stdout
            names = {ln.split()[-1] for ln in syms.splitlines() if " F " in ln and ".text" in ln}
            dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], check=True,
                                 capture_output=True, text=True).stdout
            cur = None
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
                if m:
                    cur = f"{tu}:{m.group(1)}" if m.group(1) in names else None
                    if cur:
                        assert cur not in out, cur
                        out[cur] = []
                elif cur and "//" in line:
                    out[cur].append(line.split("//")[0].strip())
    return out


if __name__ == "__main__":
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    gone, added = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    diff = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    print(f"{len(a)} kernels in {sys.argv[1]}, {len(b)} in {sys.argv[2]}: {len(set(a) & set(b)) - len(diff)} identical, "
          f"{len(diff)} different, {len(gone)} missing, {len(added)} added")
    for tag, ks in (("different", diff), ("missing", gone), ("added", added)):
        for k in ks:
            print(tag, k)
    sys.exit(1 if gone or added or diff else 0)
