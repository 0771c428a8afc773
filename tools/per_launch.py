"""Medians per (kernel, grid) of a rocprofv3 kernel trace (the format of profiles/x6_*_per_launch.txt).
Several traces (runs of one build) are pooled.
usage: per_launch.py [--keep SUBSTRING of the kernel names, default x6] <..._kernel_trace.csv> ..."""
import collections
import csv
import re
import sys

import numpy as np

args, keep = sys.argv[1:], "x6"
if args[:1] == ["--keep"]:
    keep, args = args[1], args[2:]
rows = collections.defaultdict(list)
for path in args:
    for r in csv.DictReader(open(path, newline="")):
        name = r["Kernel_Name"]
        if keep not in name:
            continue
        name = re.sub(r"\(anonymous namespace\)::", "", name.replace("void ", ""))
        name = re.sub(r"\(.*$", "", name)                       # drop the argument list
        name = re.sub(r"^esa::(?=conv_x6|stem_x6|head_x6)", "", name)
        rows[(name, int(r["Grid_Size_X"]) * int(r.get("Grid_Size_Y", 1) or 1))].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
for (name, grid), us in sorted(rows.items(), key=lambda kv: -sum(kv[1])):
    us = np.array(us)
    print(f"{name:<45s} grid={grid:>8d} launches={len(us):>5d} median_us={np.median(us):>8.1f} mean_us={us.mean():>8.1f} total_ms={us.sum() * 1e-3:>9.2f}")
