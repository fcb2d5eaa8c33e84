#!/usr/bin/env python3
"""dev tool (container): do two builds hold the same gfx950 device code?

    python tools/kernel_bytes.py A B        (A, B: a built library / object with an embedded HIP fat binary, or a gfx950 code object)

Unbundles the gfx950 image of each side, disassembles it and hashes, per symbol, the instruction ENCODINGS in order -- the
words of every instruction, no addresses, no symbol offsets (branches are relative, so a function that moved keeps its
bytes).  Prints the symbols that exist on one side only and the symbols whose encodings differ; exit status 1 if there is
any, 0 if the two sides are the same code.  The check behind "identical instruction bytes" in DESIGN.md: a refactor of the
kernels' SOURCE that passes it cannot have changed a pixel or a microsecond of device time.
"""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def llvm_tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"), "/opt/rocm/llvm/bin"):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    p = shutil.which(name)
    if not p:
        raise SystemExit(f"{name} not found (ROCm's llvm/bin)")
    return p


def code_object(path, tmp, tag):
    """the gfx950 code object of `path`: the file itself if it is one, otherwise the image of its .hip_fatbin section"""
    with open(path, "rb") as f:
        head = f.read(20)
    if head[:4] == b"\x7fELF" and int.from_bytes(head[18:20], "little") == 224:      # e_machine: EM_AMDGPU
        return path
    fat = os.path.join(tmp, tag + ".fatbin")
    if head[:4] == b"\x7fELF":
        subprocess.run([llvm_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, path, os.path.join(tmp, tag + ".copy")], check=True)
    else:
        fat = path                                                                   # a bare bundle (.hipfb)
    co = os.path.join(tmp, tag + ".co")
    subprocess.run([llvm_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fat, "--output=" + co], check=True)
    if not os.path.exists(co) or os.path.getsize(co) == 0:
        raise SystemExit(f"{path}: no {TARGET} image")
    return co


def symbol_hashes(co):
    """symbol -> (sha256 of its instruction words, number of instructions)"""
    out = subprocess.run([llvm_tool("llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
    syms, cur = {}, None
    for line in out.split("\n"):
        m = re.match(r"^[0-9a-fA-F]+ <(.+)>:$", line)
        if m:
            cur = syms.setdefault(m.group(1), [hashlib.sha256(), 0])
            continue
        m = re.search(r"// [0-9A-Fa-f]+: ((?:[0-9A-Fa-f]{8} ?)+)", line)
        if m and cur is not None:
            cur[0].update(m.group(1).strip().encode())
            cur[0].update(b"\n")
            cur[1] += 1
    return {k: (h.hexdigest(), n) for k, (h, n) in syms.items()}


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    with tempfile.TemporaryDirectory(prefix="rrt_kbytes_") as tmp:
        a, b = (symbol_hashes(code_object(p, tmp, t)) for p, t in zip(sys.argv[1:], ("a", "b")))
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(s for s in set(a) & set(b) if a[s] != b[s])
    names = only_a + only_b + differ
    pretty = dict(zip(names, subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n"))) if names and shutil.which("c++filt") else {}
    for title, group in (("only in " + sys.argv[1], only_a), ("only in " + sys.argv[2], only_b)):
        for s in group:
            print(f"{title}: {pretty.get(s, s)}")
    for s in differ:
        print(f"differs: {pretty.get(s, s)}  ({a[s][1]} instructions against {b[s][1]})")
    n_ins = sum(n for _, n in a.values())
    print(f"{len(a)} symbols ({n_ins} instructions) against {len(b)}: {len(only_a)} only in the first, {len(only_b)} only in the second, {len(differ)} differ")
    return 1 if names else 0


if __name__ == "__main__":
    sys.exit(main())
