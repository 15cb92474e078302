#!/usr/bin/env python3
"""Worst observed error of every op of the float64 numerical core over the case sets of tests/test_gpu_linalg_direct.py, one
JSON line per op (needs the GPU).  Every test of that file prints its figures before it asserts ("linalg_direct <op>[<set>]:
<figure> <value> ..."); this runs the file once, keeps the largest value of each figure per op and prints
{"op": ..., "figures": {...}, "sets": n}.  `*_eps` figures are in units of eps = 2^-52, `*_ulp` in ulp, the Kabsch offset
law's and the far-from-origin alignments' in metres / radians.  profiles/linalg_direct_errors.jsonl is its output on an MI355X.

    python tools/linalg_errors.py > profiles/linalg_direct_errors.jsonl"""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"linalg_direct (\S+?)(\[.*\])?: (.*)$")


def main():
    run = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_linalg_direct.py"), "-m", "gpu", "-s", "-q", "-p", "no:cacheprovider"],
                         cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    ops = {}
    for line in run.stdout.splitlines():
        m = LINE.search(line.lstrip("."))
        if not m:
            continue
        op, sub, rest = m.group(1), m.group(2), m.group(3).split()
        # the offset law and the far alignments are per distance: one line each, not a maximum over distances
        key = op + sub if sub and ((op == "kabsch" and sub.startswith("[offset")) or op == "far") else op
        entry = ops.setdefault(key, {"figures": {}, "sets": 0})
        entry["sets"] += 1
        for name, value in zip(rest[0::2], rest[1::2]):
            entry["figures"][name] = max(entry["figures"].get(name, float("-inf")), float(value))
    for op, entry in ops.items():
        print(json.dumps({"op": op, "figures": entry["figures"], "sets": entry["sets"]}))
    tail = run.stdout.strip().splitlines()[-1] if run.stdout.strip() else ""
    print(json.dumps({"pytest": tail, "exit": run.returncode}))
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())
