"""Micro-benchmark of HipSchurSolver.solve_multi_with_factor (thx_ba_reduce_multi + the multi-vector solve of the reduced system +
thx_ba_backsub_multi) against a loop of nrhs calls of solve_with_factor on the same factor -- the only way to a block of solves
before the kernels existed (each call rebuilds the reduced system to eliminate the points of one vector).  The objective of bench.py
(make_ba_objective, 512 cameras / 8192 points / 32768 observations); HIP events on torch's current stream, one warm-up call each,
then interleaved rounds, the median and the range reported; ``kernels``: the two new kernels alone on the same block.

usage: python tools/bench_ba_multi.py [--cams 512] [--points 8192] [--batch 64,256] [--nrhs 6,32] [--dtype f32] [--rounds 5]
                                      [--solver-kwargs '{}'] [--out FILE]
Prints one JSON line per (batch, nrhs)."""
import argparse
import json
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import theseus_amd as th
from theseus_amd.utils.synthetic_ba import make_ba_objective

ap = argparse.ArgumentParser()
ap.add_argument("--cams", type=int, default=512)
ap.add_argument("--points", type=int, default=8192)
ap.add_argument("--batch", default="64,256")
ap.add_argument("--nrhs", default="6,32")
ap.add_argument("--dtype", default="f32")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--solver-kwargs", default="{}")
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_ba_multi.py needs a HIP device"
dt = {"f32": torch.float32, "f64": torch.float64}[args.dtype]


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


lines = []
for B in (int(v) for v in args.batch.split(",")):
    obj, info = make_ba_objective(args.cams, args.points, B, dtype=dt)
    opt = th.LevenbergMarquardt(obj, max_iterations=1, linear_solver_kwargs=json.loads(args.solver_kwargs) or None)
    solver, lin = opt.linear_solver, opt.linear_solver.linearization
    obj.update()
    lin.linearize()
    solver.solve(damping=1e-2)
    K, p, n = solver.K, lin.packed, lin.n
    gen = torch.Generator(device="cuda").manual_seed(1)
    for nrhs in (int(v) for v in args.nrhs.split(",")):
        rhs = torch.randn(B, nrhs, n, dtype=dt, device="cuda", generator=gen)
        cols = [rhs[:, s].contiguous() for s in range(nrhs)]
        work, out = rhs.clone(), {}

        def multi():
            out["multi"] = solver.solve_multi_with_factor(rhs)

        def loop():
            out["loop"] = [solver.solve_with_factor(c) for c in cols]

        def kernels():   # (on a scratch block: the values do not matter, the traffic is the same)
            K.ba_reduce_multi(p.dstruct, lin.W, solver.Hinv, work, work, which=0)
            K.ba_backsub_multi(p.dstruct, lin.W, solver.Hinv, work, which=0)

        contenders = dict(multi=multi, loop=loop, kernels=kernels)
        for fn in contenders.values():     # warm-up
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in contenders}
        for _ in range(args.rounds):
            for k, fn in contenders.items():
                times[k].append(event_ms(fn))
        med = {k: statistics.median(v) for k, v in times.items()}
        agree = float((out["multi"] - torch.stack(out["loop"], dim=1)).abs().max() / out["multi"].abs().max())
        line = dict(cams=info["num_cams"], points=info["num_points"], obs=info["num_obs"], n=n, B=B, dtype=args.dtype,
                    levels=bool(solver.levels), sparse=bool(solver.sparse), nrhs=nrhs, rounds=args.rounds,
                    ms={k: [round(t, 3) for t in v] for k, v in times.items()}, ms_median={k: round(v, 3) for k, v in med.items()},
                    ms_range={k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()},
                    loop_over_multi=round(med["loop"] / med["multi"], 2), multi_vs_loop_max_rel=agree)
        print(json.dumps(line), flush=True)
        lines.append(line)
        del rhs, cols, work, out
    del solver, opt, obj
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
