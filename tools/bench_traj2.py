"""ms per LM iteration of a 2D motion-planning objective (Collision2D + GPMotionModel + boundary priors, examples/
motion_planning_2d.py) on the fused family (PackedTrajectory2D: thx_traj2_eval / thx_traj2_error) and on the generic path
(PackedEuclidean: every cost evaluated by torch) -- same objective, same kernels downstream, interleaved on one device.

    python tools/bench_traj2.py --intervals 100 --batch 64 1024 --dtype f32 --iters 10 --repeats 7 [--out profiles/traj2/x.jsonl]

One JSON line per batch size: median / min ms per iteration of both paths, their ratio, and the device kernels per iteration
(torch.profiler; None when the profiler is unavailable)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from examples.motion_planning_2d import make_objective  # noqa: E402


def optimizer(th, N, B, dtype, fused, iters):
    obj = make_objective(th, N, B, dtype, "cuda")
    if not fused:
        from theseus_amd.euclidean import PackedEuclidean
        obj._packed = PackedEuclidean(obj)      # packed_for() keeps a packed representation that is current
    opt = th.LevenbergMarquardt(obj, max_iterations=iters, step_size=1.0, abs_err_tolerance=0.0, rel_err_tolerance=0.0)
    want = "PackedTrajectory2D" if fused else "PackedEuclidean"
    assert type(opt.linear_solver.linearization.packed).__name__ == want
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


def kernels_per_iteration(obj, opt, start, iters):
    try:
        from torch.profiler import ProfilerActivity, profile
        counts = []
        short = (2, 2, 4)   # a throw-away pass, then the difference of two short runs: per-iteration launches without the set-up
        for k in short:
            opt.params.max_iterations = k
            obj.update({n: v.clone() for n, v in start.items()})
            with profile(activities=[ProfilerActivity.CUDA]) as prof, torch.no_grad():
                opt.optimize(damping=0.1)
                torch.cuda.synchronize()
            counts.append(sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA))
        opt.params.max_iterations = iters
        per_iter = (counts[2] - counts[1]) / (short[2] - short[1])
        return per_iter if per_iter > 0 else None   # (a pass in which the profiler dropped events)
    except Exception as exc:   # noqa: BLE001  (the count is a diagnostic: the timings stand without it)
        print(f"[bench_traj2] kernel count unavailable: {exc}", file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--intervals", type=int, default=100)
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f32")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import theseus_amd as th
    dtype = torch.float32 if a.dtype == "f32" else torch.float64
    for B in a.batch:
        paths = {"fused": optimizer(th, a.intervals, B, dtype, True, a.iters), "generic": optimizer(th, a.intervals, B, dtype, False, a.iters)}
        for _ in range(a.warmup):
            for p in paths.values():
                run(*p)
        ms = {k: [] for k in paths}
        for _ in range(a.repeats):          # interleaved: both paths see the same clocks
            for k, p in paths.items():
                ms[k].append(run(*p) / a.iters)
        final = {k: float(p[0].error_metric().mean()) for k, p in paths.items()}
        launches = {k: kernels_per_iteration(*p, a.iters) for k, p in paths.items()}
        rec = dict(intervals=a.intervals, n=4 * (a.intervals + 1), costs=len(paths["fused"][0].cost_functions), batch=B, dtype=a.dtype,
                   iters=a.iters, repeats=a.repeats,
                   fused_ms_per_iter=statistics.median(ms["fused"]), fused_min=min(ms["fused"]),
                   generic_ms_per_iter=statistics.median(ms["generic"]), generic_min=min(ms["generic"]),
                   speedup=statistics.median(ms["generic"]) / statistics.median(ms["fused"]),
                   kernels_per_iter_fused=launches["fused"], kernels_per_iter_generic=launches["generic"],
                   final_error_fused=final["fused"], final_error_generic=final["generic"], device=torch.cuda.get_device_name(0))
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
