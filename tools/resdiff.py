#!/usr/bin/env python
"""Side-by-side kernel resources of two -Rpass-analysis remark files (tools/resources.sh): resdiff.py old.txt new.txt [regex]
Only kernels whose SGPR / VGPR / occupancy / LDS / scratch differ are printed."""
import re, subprocess, sys

def parse(path):
    cur, rows = None, {}
    for l in open(path):
        m = re.search(r"Function Name: (\S+)", l)
        if m:
            cur = m.group(1); rows[cur] = {}
        for key, short in (("SGPRs", "s"), ("VGPRs", "v"), ("Occupancy", "occ"), ("LDS Size", "lds"), ("ScratchSize", "scr")):
            m = re.search(key + r"[^:]*: (\d+)", l)
            if m and cur: rows[cur].setdefault(short, int(m.group(1)))
    return rows
a, b = parse(sys.argv[1]), parse(sys.argv[2])
pat = re.compile(sys.argv[3]) if len(sys.argv) > 3 else None
def demangled(rows):  # keyed by the demangled name without its parameter list: a kernel that only gained a trailing (empty) parameter pack keeps its key
    names = list(rows)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {d.split("(")[0].replace("void cmax::", ""): rows[k] for k, d in zip(names, dem)}
a, b = demangled(a), demangled(b)
for d in sorted(set(a) | set(b)):
    if pat and not pat.search(d): continue
    if a.get(d) != b.get(d): print(f"{d:56s} {a.get(d)} -> {b.get(d)}")
