"""Micro-benchmark of HipSparseCholeskySolver.solve_multi_with_factor (thx_chol_solve_multi_sparse) against a loop of nrhs calls of
solve_with_factor on the same factor -- the only way to a block of solves before the kernel existed.  The chain graph of
examples/large_pose_graph.py; HIP events on torch's current stream, one warm-up call each, then interleaved rounds, the median
reported.

usage: python tools/bench_sparse_multi.py [--poses 4096] [--batch 8,64] [--nrhs 6,32,256] [--ordering rcm,nd] [--dtype f32]
                                          [--rounds 5] [--out FILE]
Prints one JSON line per (ordering, batch, nrhs).  ``L_TB_per_s``: terabytes of L and of solve panels the multi call streams (every
tile of the pattern, once per substitution and group of 32 vectors) over the median time, beside the 8 TB/s HBM peak;
``workgroups``: batch x groups, what the single launch spreads over the 256 CUs."""
import argparse
import json
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import theseus_amd as th
from theseus_amd.utils.synthetic import chain_graph_topology

HBM = 8e12   # MI355X: HBM3E 8 TB/s

ap = argparse.ArgumentParser()
ap.add_argument("--poses", type=int, default=4096)
ap.add_argument("--batch", default="8,64")
ap.add_argument("--nrhs", default="6,32,256")
ap.add_argument("--ordering", default="rcm,nd")
ap.add_argument("--dtype", default="f32")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_sparse_multi.py needs a HIP device"
dt = {"f32": torch.float32, "f64": torch.float64}[args.dtype]
esize, P = (4 if dt == torch.float32 else 8), args.poses


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def factored_solver(B, ordering):
    """The example's objective, linearized and factorised once with the example's damping."""
    K = th.default_kernels()
    edges = chain_graph_topology(P, stride=7, span=5, seed=2, shuffle=True)
    gen = torch.Generator(device="cuda").manual_seed(7)
    rnd = lambda n, s: K.se3_exp(s * (2 * torch.rand(n, 6, dtype=dt, device="cuda", generator=gen) - 1))  # noqa: E731
    gt = rnd(B * P, 1.5).view(B, P, 3, 4)
    poses0 = K.se3_compose(gt.reshape(-1, 3, 4), rnd(B * P, 0.05)).view(B, P, 3, 4)
    obj = th.Objective(dtype=dt)
    pv = [th.SE3(tensor=poses0[:, k].clone(), name=f"pose_{k}") for k in range(P)]
    w = th.ScaleCostWeight(torch.tensor(5.0, dtype=dt, device="cuda"))
    for k, (i, j) in enumerate(edges):
        z = K.se3_compose(K.se3_compose(K.se3_inverse(gt[:, i].contiguous()), gt[:, j].contiguous()), rnd(B, 0.01))
        obj.add(th.Between(pv[i], pv[j], th.SE3(tensor=z, name=f"z_{k}"), w, name=f"between_{k}"))
    obj.add(th.Difference(pv[edges[0][0]], th.SE3(tensor=gt[:, edges[0][0]].clone(), name="anchor"), w, name="prior"))
    solver = th.HipSparseCholeskySolver(obj, ordering=ordering)
    solver.linearization.linearize()
    solver.solve(damping=1e-2)
    return solver


lines = []
for ordering in args.ordering.split(","):
    for B in (int(v) for v in args.batch.split(",")):
        solver = factored_solver(B, ordering)
        pat, n = solver.pattern, solver.linearization.n
        gen = torch.Generator(device="cuda").manual_seed(1)
        for nrhs in (int(v) for v in args.nrhs.split(",")):
            rhs = torch.randn(B, nrhs, n, dtype=dt, device="cuda", generator=gen)
            cols = [rhs[:, s].contiguous() for s in range(nrhs)]
            out = {}

            def multi():
                out["multi"] = solver.solve_multi_with_factor(rhs)

            def loop():
                out["loop"] = [solver.solve_with_factor(c) for c in cols]

            contenders = dict(multi=multi, loop=loop)
            for fn in contenders.values():     # warm-up
                fn()
            torch.cuda.synchronize()
            times = {k: [] for k in contenders}
            for _ in range(args.rounds):
                for k, fn in contenders.items():
                    times[k].append(event_ms(fn))
            med = {k: statistics.median(v) for k, v in times.items()}
            agree = float((out["multi"] - torch.stack(out["loop"], dim=1)).abs().max() / out["multi"].abs().max())
            groups = (nrhs + 31) // 32
            l_bytes = 2.0 * B * groups * pat.l_tiles * 128 * 128 * esize      # forward + backward; diagonal tiles through the panels
            line = dict(poses=P, n=n, B=B, dtype=args.dtype, ordering=ordering, levels=bool(solver.levels), tiles=pat.ntiles,
                        l_tiles=pat.l_tiles, nrhs=nrhs, workgroups=B * groups, rounds=args.rounds,
                        ms={k: [round(t, 3) for t in v] for k, v in times.items()}, ms_median={k: round(v, 3) for k, v in med.items()},
                        loop_over_multi=round(med["loop"] / med["multi"], 2), multi_vs_loop_max_rel=agree,
                        L_TB_per_s=round(l_bytes / (med["multi"] * 1e-3) / 1e12, 3),
                        L_fraction_of_hbm_peak=round(l_bytes / (med["multi"] * 1e-3) / HBM, 4))
            print(json.dumps(line), flush=True)
            lines.append(line)
            del rhs, cols, out
        del solver
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
