"""Per-launch time of chol_offdiag2_f32_kernel by column pair, from a rocprofv3 kernel trace of bench.py (the csv of
``rocprofv3 --kernel-trace --output-format csv``).  The launches of one pair differ from the other pairs' by their grid: a pair
(j, j + 1) of an ntiles-tile factor has ntiles - 2 - j row tiles (or row groups) per problem, so the grids descend with j.
usage: python tools/pair_launch_times.py <kernel_trace.csv>"""
import csv
import sys
from collections import defaultdict

by_grid = defaultdict(list)
for r in csv.DictReader(open(sys.argv[1])):
    if "chol_offdiag2_f32_kernel" in r["Kernel_Name"]:
        grid = int(r["Grid_Size_X"]) // max(1, int(r["Workgroup_Size_X"]))
        by_grid[grid].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
print(f"{'pair':>6s} {'workgroups':>11s} {'launches':>9s} {'avg_us':>10s} {'min_us':>10s} {'max_us':>10s}")
total = 0.0
for k, grid in enumerate(sorted(by_grid, reverse=True)):
    t = by_grid[grid]
    total += sum(t)
    print(f"j={2 * k:<4d} {grid:11d} {len(t):9d} {sum(t) / len(t):10.1f} {min(t):10.1f} {max(t):10.1f}")
print(f"all pairs: {total / 1e3:.3f} ms of kernel time over {sum(len(t) for t in by_grid.values())} launches")
