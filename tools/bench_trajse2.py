"""ms per LM iteration of the SE2 motion planner's objective (examples/se2_planning.py: Collision2D + GPMotionModel on SE2,
Nonholonomic, HingeCost, the four boundary priors) on the fused path (PackedTrajectorySE2: thx_trajse2_eval / thx_trajse2_error /
thx_trajse2_retract) and on the SAME packed class with the fused evaluation switched off (``packed.fused = False``: every cost
evaluated by its torch class) -- same objective, same kernels downstream, interleaved on one device.

    python tools/bench_trajse2.py --intervals 100 --batch 64 1024 --dtype f32 --iters 20 --repeats 7 [--out profiles/trajse2/x.jsonl]

One JSON line per batch size: median / min ms per iteration of both paths, their ratio and the final objectives of both."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from examples.se2_planning import make_objective  # noqa: E402


def optimizer(th, N, B, dtype, fused, iters):
    obj = make_objective(th, N, B, dtype, "cuda")
    opt = th.LevenbergMarquardt(obj, max_iterations=iters, step_size=0.25, abs_err_tolerance=0.0, rel_err_tolerance=0.0)
    packed = opt.linear_solver.linearization.packed
    assert type(packed).__name__ == "PackedTrajectorySE2"
    packed.fused = fused
    start = {k: v.tensor.clone() for k, v in obj.optim_vars.items()}
    return obj, opt, start


def run(obj, opt, start):
    obj.update({k: v.clone() for k, v in start.items()})
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        opt.optimize(damping=0.1)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--intervals", type=int, default=100)
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f32")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import theseus_amd as th
    dtype = torch.float32 if a.dtype == "f32" else torch.float64
    for B in a.batch:
        paths = {"fused": optimizer(th, a.intervals, B, dtype, True, a.iters), "torch": optimizer(th, a.intervals, B, dtype, False, a.iters)}
        for _ in range(a.warmup):
            for p in paths.values():
                run(*p)
        ms = {k: [] for k in paths}
        for _ in range(a.repeats):          # interleaved: both paths see the same clocks
            for k, p in paths.items():
                ms[k].append(run(*p) / a.iters)
        final = {k: float(p[1].linear_solver.linearization.packed.error_metric().mean()) for k, p in paths.items()}
        rec = dict(intervals=a.intervals, n=6 * (a.intervals + 1), costs=len(paths["fused"][0].cost_functions), batch=B, dtype=a.dtype,
                   iters=a.iters, warmup=a.warmup, repeats=a.repeats,
                   fused_ms_per_iter=statistics.median(ms["fused"]), fused_min=min(ms["fused"]),
                   torch_ms_per_iter=statistics.median(ms["torch"]), torch_min=min(ms["torch"]),
                   speedup=statistics.median(ms["torch"]) / statistics.median(ms["fused"]),
                   final_error_fused=final["fused"], final_error_torch=final["torch"], device=torch.cuda.get_device_name(0))
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
