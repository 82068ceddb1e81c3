"""chol_syrk_kernel launches of every factor call of a rocprofv3 kernel trace (tools/summarize_prof.py's directory layout) in start
order: two per block column and call at the headline batch (block column j = position // 2, the two half-batch streams alternate);
mean duration per j over the calls.
usage: python tools/syrk_launch_times.py <dir with trace/**/*kernel_trace.csv>"""
import csv, glob, os, sys
from collections import defaultdict
out = sys.argv[1]
f = glob.glob(os.path.join(out, "trace/**/*kernel_trace.csv"), recursive=True)[0]
rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
calls, cur = [], []
for r in rows:
    n = r["Kernel_Name"]
    if "chol_syrk_kernel" in n:
        cur.append((n.split("(")[0].replace("void thx::", ""), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    elif "chol_bwd" in n and cur:
        calls.append(cur); cur = []
if cur: calls.append(cur)
# the mapping position -> block column assumes that the two streams alternate column by column (the second half batch runs one diagonal
# phase behind the first and both wait for the same off-diagonal launches).  Checked as far as the trace allows: every call has the same
# even number of launches, and both launches of a position pair are the same instantiation in every call.
assert len({len(c) for c in calls}) == 1 and len(calls[0]) % 2 == 0, [len(c) for c in calls]
for c in calls:
    assert all(c[2 * k][0] == c[2 * k + 1][0] == calls[0][2 * k][0] for k in range(len(c) // 2)), "the streams do not alternate"
print(f"== chol_syrk_kernel per block column (us per launch, mean over {len(calls)} calls x 2 streams; {len(calls[0])} launches per call) ==")
per = defaultdict(list)
for c in calls:
    for p, (n, d) in enumerate(c):
        per[(p // 2, n)].append(d)
for (j, n), v in sorted(per.items()):
    print(f"j={j:2d} {n:40s} {sum(v) / len(v) / 1e3:9.1f}")
print(f"per call: {sum(d for c in calls for _, d in c) / len(calls) / 1e6:.3f} ms")
