#!/usr/bin/env python3
"""Reduce the output of `make resources` (stdin) to one sorted line per kernel: the demangled name with the parameter list cut off, then
TotalSGPRs, VGPRs, AGPRs, ScratchSize, Occupancy, SGPRs Spill, VGPRs Spill and LDS Size.  Source locations are dropped, so two builds
compare with diff:  make resources 2>&1 | tools/resources_reduce.py > a.txt"""
import re
import subprocess
import sys

KEYS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize", "Occupancy", "SGPRs Spill", "VGPRs Spill", "LDS Size")
rows, cur = [], None
for line in sys.stdin:
    m = re.search(r"remark:\s+(.*?)\s*\[-Rpass-analysis", line)
    if not m:
        continue
    text = m.group(1)
    if text.startswith("Function Name:"):
        cur = [text.split(":", 1)[1].strip(), {}]
        rows.append(cur)
    elif cur is not None and ":" in text:
        key, value = text.rsplit(":", 1)
        key = re.sub(r"\s*\[.*\]", "", key).strip()
        if key in KEYS:
            cur[1][key] = value.strip()
names = subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True, text=True, check=True).stdout.split("\n")
out = []
for (_, fig), name in zip(rows, names):
    name = re.sub(r"^void ", "", name)
    out.append(name.split("(", 1)[0] + "  " + ", ".join(f"{k} {fig.get(k, '?')}" for k in KEYS))
print("\n".join(sorted(out)))
