"""ms per LM iteration of the planar-pushing pose estimator's objective (examples/planar_pushing.py: QuasiStaticPushingPlanar +
MovingFrameBetween + EffectorObjectContactPlanar + SE2 priors) on the fused path (PackedPlanarPushing: thx_push2_eval /
thx_push2_error) and on the SAME packed class with the fused evaluation switched off (``packed.fused = False``: every cost evaluated
by its torch class) -- same objective, same kernels downstream, interleaved on one device.

    python tools/bench_push2.py --steps 25 --batch 64 1024 --dtype f32 --iters 20 --repeats 7 [--out profiles/push2/x.jsonl]

One JSON line per batch size: median / min ms per iteration of both paths, their ratio, and the device kernels per iteration
(torch.profiler).  A pass without a valid count is recorded as such and the run exits non-zero."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from examples.planar_pushing import make_objective  # noqa: E402


def optimizer(th, T, B, dtype, fused, iters):
    obj, _ = make_objective(th, T, B, dtype, "cuda")
    opt = th.LevenbergMarquardt(obj, max_iterations=iters, step_size=1.0, abs_err_tolerance=0.0, rel_err_tolerance=0.0)
    packed = opt.linear_solver.linearization.packed
    assert type(packed).__name__ == "PackedPlanarPushing"
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


def kernels_per_iteration(obj, opt, start, iters):
    """device kernels per LM iteration (torch.profiler): the difference of a 2- and a 1-iteration run, after a throw-away pass
    (short runs: the tracer drops events beyond a few ten thousand per pass).  -> (count | None, events per pass)"""
    from torch.profiler import ProfilerActivity, profile
    counts = []
    short = (1, 1, 2)
    for k in short:
        opt.params.max_iterations = k
        obj.update({n: v.clone() for n, v in start.items()})
        with profile(activities=[ProfilerActivity.CUDA]) as prof, torch.no_grad():
            opt.optimize(damping=0.1)
            torch.cuda.synchronize()
        counts.append(sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA))
    opt.params.max_iterations = iters
    per_iter = (counts[2] - counts[1]) / (short[2] - short[1])
    return (per_iter if per_iter > 0 and counts[0] == counts[1] else None), counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f32")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import theseus_amd as th
    dtype = torch.float32 if a.dtype == "f32" else torch.float64
    missing = []
    for B in a.batch:
        paths = {"fused": optimizer(th, a.steps, B, dtype, True, a.iters), "torch": optimizer(th, a.steps, B, dtype, False, a.iters)}
        for _ in range(a.warmup):
            for p in paths.values():
                run(*p)
        ms = {k: [] for k in paths}
        for _ in range(a.repeats):          # interleaved: both paths see the same clocks
            for k, p in paths.items():
                ms[k].append(run(*p) / a.iters)
        final = {k: float(p[1].linear_solver.linearization.packed.error_metric().mean()) for k, p in paths.items()}
        launches = {k: kernels_per_iteration(*p, a.iters) for k, p in paths.items()}
        rec = dict(steps=a.steps, n=6 * a.steps, costs=len(paths["fused"][0].cost_functions), batch=B, dtype=a.dtype,
                   iters=a.iters, repeats=a.repeats,
                   fused_ms_per_iter=statistics.median(ms["fused"]), fused_min=min(ms["fused"]),
                   torch_ms_per_iter=statistics.median(ms["torch"]), torch_min=min(ms["torch"]),
                   speedup=statistics.median(ms["torch"]) / statistics.median(ms["fused"]),
                   kernels_per_iter_fused=launches["fused"][0], kernels_per_iter_torch=launches["torch"][0],
                   profiler_events_per_pass={k: v[1] for k, v in launches.items()},
                   final_error_fused=final["fused"], final_error_torch=final["torch"], device=torch.cuda.get_device_name(0))
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
        missing += [f"{k} at batch {B}" for k, v in launches.items() if v[0] is None]
    if missing:
        sys.exit(f"bench_push2: no valid kernel count for {', '.join(missing)} (the timings above stand)")


if __name__ == "__main__":
    main()
