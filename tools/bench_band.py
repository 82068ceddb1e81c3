"""The banded Cholesky solver (HipBandedCholeskySolver) against the dense one (HipCholeskySolver) on the 2D motion planner of
examples/motion_planning_2d.py -- same objective, same fused cost family, same assembly; only ``linear_solver_cls`` differs.  The
protocol of tools/bench_traj2.py: both on one device, interleaved, 2 warm-ups, median of 7 repeats, fp32, 20 LM iterations per
``optimize()``.

    python tools/bench_band.py --intervals 100 --batch 64 1024 [--long 1000 --long-batch 64] [--out profiles/band/x.jsonl]

One JSON line per batch size with
  * ms per LM iteration of both solvers, median and min .. max of the repeats;
  * ms of the linear solve alone -- factor + both substitutions, ``solver.solve(damping)`` on the last linearization, timed over
    ``--solve-reps`` back-to-back calls between two synchronisations -- of both solvers;
  * ``solve_faster`` / ``iter_faster``: the banded median lies below the dense one by more than the dense runs' own min .. max spread;
and, with ``--long N``, one line for the banded solver alone at that horizon (the dense solver's cost grows as N^3)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from examples.motion_planning_2d import make_objective  # noqa: E402


def optimizer(th, N, B, dtype, solver_cls, iters):
    obj = make_objective(th, N, B, dtype, "cuda")
    opt = th.LevenbergMarquardt(obj, linear_solver_cls=solver_cls, max_iterations=iters, step_size=1.0, abs_err_tolerance=0.0,
                                rel_err_tolerance=0.0)
    assert type(opt.linear_solver.linearization.packed).__name__ == "PackedTrajectory2D" and type(opt.linear_solver) is solver_cls
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


def solve_alone(opt, reps):
    """ms per ``solve()`` on the linearization as the last optimize() left it (check_info=False: no host look in between)."""
    solver = opt.linear_solver
    with torch.no_grad():
        solver.linearization.linearize()
        solver.solve(damping=0.1, check_info=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            solver.solve(damping=0.1, check_info=False)
        torch.cuda.synchronize()
    assert int(solver.info.ne(0).sum()) == 0
    return (time.perf_counter() - t0) * 1e3 / reps


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def faster(banded, dense):
    """the banded median is below the dense median by more than the dense runs' own min .. max spread"""
    return bool(dense["median"] - banded["median"] > dense["max"] - dense["min"])


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--intervals", type=int, default=100)
    ap.add_argument("--batch", type=int, nargs="*", default=[64, 1024])
    ap.add_argument("--long", type=int, default=0, help="a horizon for the banded solver alone (0: skip)")
    ap.add_argument("--long-batch", type=int, default=64)
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f32")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--solve-reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import theseus_amd as th
    dtype = torch.float32 if a.dtype == "f32" else torch.float64
    common = dict(dtype=a.dtype, iters=a.iters, repeats=a.repeats, warmup=a.warmup, solve_reps=a.solve_reps,
                  device=torch.cuda.get_device_name(0))
    for B in a.batch:
        paths = {"dense": optimizer(th, a.intervals, B, dtype, th.HipCholeskySolver, a.iters),
                 "banded": optimizer(th, a.intervals, B, dtype, th.HipBandedCholeskySolver, a.iters)}
        for _ in range(a.warmup):
            for p in paths.values():
                run(*p)
        it, sv = {k: [] for k in paths}, {k: [] for k in paths}
        for _ in range(a.repeats):          # interleaved: both solvers see the same clocks
            for k, p in paths.items():
                it[k].append(run(*p) / a.iters)
            for k, p in paths.items():
                sv[k].append(solve_alone(p[1], a.solve_reps))
        it, sv = {k: stats(v) for k, v in it.items()}, {k: stats(v) for k, v in sv.items()}
        plan = paths["banded"][1].linear_solver.band_plan()
        emit(dict(what="dense_vs_banded", intervals=a.intervals, n=plan.n, kd=plan.kd, batch=B,
                  iter_ms_dense=it["dense"], iter_ms_banded=it["banded"], iter_faster=faster(it["banded"], it["dense"]),
                  solve_ms_dense=sv["dense"], solve_ms_banded=sv["banded"], solve_faster=faster(sv["banded"], sv["dense"]),
                  final_error_dense=float(paths["dense"][0].error_metric().mean()),
                  final_error_banded=float(paths["banded"][0].error_metric().mean()), **common), a.out)
        del paths
        torch.cuda.empty_cache()
    if a.long:
        p = optimizer(th, a.long, a.long_batch, dtype, th.HipBandedCholeskySolver, a.iters)
        for _ in range(a.warmup):
            run(*p)
        it, sv = [], []
        for _ in range(a.repeats):
            it.append(run(*p) / a.iters)
            sv.append(solve_alone(p[1], a.solve_reps))
        plan = p[1].linear_solver.band_plan()
        emit(dict(what="banded_alone", intervals=a.long, n=plan.n, kd=plan.kd, batch=a.long_batch, iter_ms_banded=stats(it),
                  solve_ms_banded=stats(sv), final_error_banded=float(p[0].error_metric().mean()), **common), a.out)


if __name__ == "__main__":
    main()
