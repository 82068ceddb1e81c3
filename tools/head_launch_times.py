"""chol_offdiag_f32_kernel launches (the column pairs' head tiles) of every factor call of a one-stream kernel trace, in start
order: the k-th launch of a call is head tile (2 k + 1, 2 k); mean duration per j over the calls.  ONE stream only (below 1024
problems per call): on two streams the two half batches' launches interleave.
usage: python tools/head_launch_times.py <dir with trace/**/*kernel_trace.csv>"""
import csv, glob, os, sys
from collections import defaultdict
out = sys.argv[1]
f = glob.glob(os.path.join(out, "trace/**/*kernel_trace.csv"), recursive=True)[0]
rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
calls, cur = [], []
for r in rows:
    n = r["Kernel_Name"]
    if "chol_offdiag_f32_kernel" in n:
        cur.append((n.split("(")[0].replace("void thx::", ""), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    elif "chol_bwd" in n and cur:
        calls.append(cur); cur = []
if cur: calls.append(cur)
assert len({len(c) for c in calls}) == 1, [len(c) for c in calls]
print(f"== head tiles (chol_offdiag_f32_kernel) per pair, us per launch, mean over {len(calls)} calls; {len(calls[0])} launches per call ==")
per = defaultdict(list)
for c in calls:
    for p, (n, d) in enumerate(c):
        per[(2 * p, n)].append(d)
for (j, n), v in sorted(per.items()):
    print(f"j={j:2d} {n:40s} {sum(v) / len(v) / 1e3:9.1f}")
print(f"per call: {sum(d for c in calls for _, d in c) / len(calls) / 1e6:.3f} ms")
