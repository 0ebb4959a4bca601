#!/usr/bin/env python
"""The head of a kernel as compiled: its memory instructions and waits (with --branches: branches too) in program order, from entry to
the first barrier; the number in front is the instruction's position in the kernel.
   python tools/head_listing.py [--branches] OBJECT REGEX [REGEX ...]
OBJECT: what `hipcc --cuda-device-only -c` wrote for a unit (tools/resources.sh keeps them with a second argument) or a code object;
REGEX: matched against the DEMANGLED kernel names.  The first 256 bytes of a kernel with preloaded arguments are the loads a
firmware without the preload runs instead; they are skipped."""
import atexit
import os
import re
import subprocess
import sys
import tempfile

ROCM_LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
KEEP = re.compile(r"^(s_load|s_buffer_load|global_load|global_store|global_atomic|buffer_|flat_|scratch_|s_waitcnt|s_barrier|s_endpgm)")
BRANCH = re.compile(r"^(s_cbranch|s_branch)")


def code_object(path):
    """`path` itself when it is a code object, else the gfx950 code object unbundled from it into a temporary file (removed at exit)."""
    with open(path, "rb") as f:
        if f.read(4) == b"\x7fELF":
            return path
    out = tempfile.NamedTemporaryFile(suffix=".co", delete=False).name
    atexit.register(os.remove, out)
    subprocess.check_call([os.path.join(ROCM_LLVM, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={path}",
                           f"--output={out}", "--unbundle"])
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "--branches"]
    branches = "--branches" in sys.argv
    co = code_object(args[0])
    pats = [re.compile(p) for p in args[1:]]
    syms = subprocess.run([os.path.join(ROCM_LLVM, "llvm-readelf"), "-s", "--wide", co], capture_output=True, text=True, check=True).stdout.split("\n")
    funcs = [l.split() for l in syms if " FUNC " in l]
    names, sizes = [f[7] for f in funcs], {f[7]: int(f[2]) for f in funcs}
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    seen = set()
    for name, d in zip(names, dem):
        if name in seen or not any(p.search(d) for p in pats):  # (.symtab and .dynsym list a kernel twice)
            continue
        seen.add(name)
        txt = subprocess.run([os.path.join(ROCM_LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", f"--disassemble-symbols={name}", co],
                             capture_output=True, text=True, check=True).stdout.split("\n")
        body = [l for l in txt if l.startswith("\t")]
        print(f"== {d.split('(')[0]}   ({sizes[name]} bytes)")
        addr0, n = None, 0
        for l in body:
            ins = l.strip().split("//")[0].strip()
            m = re.search(r"//\s*([0-9A-Fa-f]+):", l)
            addr = int(m.group(1), 16) if m else None
            if addr0 is None:
                addr0 = addr
            n += 1
            if addr is not None and addr - addr0 < 256:
                continue
            if KEEP.match(ins) or (branches and BRANCH.match(ins)):
                ins = re.sub(r"\s*<.*$", "", ins)
                print(f"  {n:5d}  {ins}")
            if ins.startswith("s_barrier"):
                break
        print()


if __name__ == "__main__":
    main()
