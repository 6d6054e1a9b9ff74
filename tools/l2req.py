#!/usr/bin/env python3
"""Summarise rocprofv3 --pmc passes of L2 request counters (no tracing beside them) per GEMM launch.

Each LABEL=DIR[,DIR...] names one build and the output directories of its counter passes; the value of
a counter is the median over the launches of each (kernel, grid) pair, as in tools/pmc.py. Counters are
written as collected (FETCH_SIZE in KiB, not doubled). Usage:
    python3 tools/l2req.py profiles/rNN_l2_requests.json parent=OUT/l2_p_a,OUT/l2_p_b head=OUT/l2_h_a,OUT/l2_h_b
"""
import collections
import csv
import glob
import json
import sys

from pmc import med, short


def load(dirs):
    out = collections.defaultdict(lambda: collections.defaultdict(list))
    for d in dirs:
        for path in glob.glob(f"{d}/**/*counter_collection.csv", recursive=True):
            for r in csv.DictReader(open(path)):
                out[(short(r["Kernel_Name"]), int(r["Grid_Size"]))][r["Counter_Name"]].append(float(r["Counter_Value"]))
    return out


def main(dst, specs):
    res = {}
    for spec in specs:
        label, dirs = spec.split("=", 1)
        rows = []
        for (kernel, grid), ctr in sorted(load(dirs.split(",")).items()):
            rows.append({"kernel": kernel, "grid": grid, "launches": min(len(v) for v in ctr.values()),
                         "counters": {k: med(v) for k, v in sorted(ctr.items())}})
        res[label] = rows
        for r in rows:
            print(label, r["grid"], r["kernel"][:110], r["counters"])
    json.dump({"note": "median per launch of each (kernel, grid); FETCH_SIZE in KiB as reported", "builds": res},
              open(dst, "w"), indent=1)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
