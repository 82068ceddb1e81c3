"""2D motion planning (GPMP2-style, the reference's examples/motion_planning_2d.py and tutorials 04 / 05) on theseus_amd's own API:
a batch of point robots crossing a map of discs.  Collision2D on every pose, GPMotionModel between consecutive (pose, velocity)
pairs, Difference priors on the start and goal states; straight-line initialisation; Levenberg-Marquardt on the fused path
(theseus_amd/embodied.py: PackedTrajectory2D -- thx_traj2_eval + thx_block_assemble + the tiled Cholesky at n = 4 (N + 1)).
The map is synthetic: the analytic signed distance of a few discs sampled on a grid (no dataset file).
usage: python examples/motion_planning_2d.py [--intervals 100] [--batch 16] [--iters 30] [--device cuda] [--dtype f64]
       (--kernels module:Class substitutes the kernel set -- the tests' CPU stand-in, for machines without a GPU)
"""
import argparse
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import theseus_amd as th  # noqa: E402

DISCS = ((-0.4, 0.15, 0.45), (0.7, -0.35, 0.4), (0.2, 0.9, 0.3))   # (cx, cy, radius)
ORIGIN, CELL, ROWS, COLS = (-2.0, -2.0), 0.05, 80, 80
TOTAL_TIME = 10.0


def disc_map(dtype, device):
    xs = ORIGIN[0] + CELL * torch.arange(COLS, dtype=dtype, device=device)
    ys = ORIGIN[1] + CELL * torch.arange(ROWS, dtype=dtype, device=device)
    Y, X = torch.meshgrid(ys, xs, indexing="ij")      # rows are y, columns are x
    return torch.stack([torch.hypot(X - cx, Y - cy) - r for cx, cy, r in DISCS]).min(dim=0).values.unsqueeze(0)


def make_objective(th, N, B, dtype, device, seed=0):
    """N intervals (N + 1 poses and velocities, n = 4 (N + 1) columns), B problems with their own start / goal."""
    gen = torch.Generator().manual_seed(seed)
    t = lambda *v: torch.tensor(v, dtype=dtype, device=device)  # noqa: E731
    start = (t(-1.6, -0.6) + 0.4 * (torch.rand(B, 2, generator=gen) - 0.5).to(dtype).to(device))
    goal = (t(1.5, 0.5) + 0.4 * (torch.rand(B, 2, generator=gen) - 0.5).to(dtype).to(device))
    dt_val = TOTAL_TIME / N
    origin = th.Point2(tensor=t(*ORIGIN).view(1, 2), name="sdf_origin")
    cell = th.Variable(t(CELL).view(1, 1), name="cell_size")
    sdf = th.Variable(disc_map(dtype, device), name="sdf_data")
    eps = th.Variable(t(0.3).view(1, 1), name="cost_eps")
    dt = th.Variable(t(dt_val).view(1, 1), name="dt")
    gp_w = th.eb.GPCostWeight(th.Variable(torch.eye(2, dtype=dtype, device=device).unsqueeze(0), name="Qc_inv"), dt)
    w_col = th.ScaleCostWeight(th.Variable(t(20.0).view(1, 1), name="w_collision"))
    w_bound = th.ScaleCostWeight(th.Variable(t(100.0).view(1, 1), name="w_boundary"))
    s = torch.linspace(0, 1, N + 1, dtype=dtype, device=device).view(1, -1, 1)
    line = start.unsqueeze(1) * (1 - s) + goal.unsqueeze(1) * s                      # straight-line initialisation
    vel = ((goal - start) / TOTAL_TIME)
    poses = [th.Point2(tensor=line[:, i].contiguous(), name=f"pose_{i}") for i in range(N + 1)]
    vels = [th.Vector(tensor=vel.clone(), name=f"vel_{i}") for i in range(N + 1)]
    zero = th.Vector(tensor=torch.zeros(1, 2, dtype=dtype, device=device), name="zero_vel")
    obj = th.Objective(dtype=dtype)
    obj.add(th.Difference(poses[0], th.Point2(tensor=start, name="start"), w_bound, name="prior_start"))
    obj.add(th.Difference(vels[0], zero, w_bound, name="prior_start_vel"))
    obj.add(th.Difference(poses[N], th.Point2(tensor=goal, name="goal"), w_bound, name="prior_goal"))
    obj.add(th.Difference(vels[N], zero, w_bound, name="prior_goal_vel"))
    for i in range(1, N):
        obj.add(th.eb.Collision2D(poses[i], origin, sdf, cell, eps, w_col, name=f"collision_{i}"))
    for i in range(N):
        obj.add(th.eb.GPMotionModel(poses[i], vels[i], poses[i + 1], vels[i + 1], dt, gp_w, name=f"gp_{i}"))
    return obj


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--intervals", type=int, default=100)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f64")
    ap.add_argument("--kernels", default=None)
    ap.add_argument("--solver", choices=["dense", "banded"], default="dense",
                    help="banded: HipBandedCholeskySolver (the chain's Hessian is banded after a reordering of its variables)")
    a = ap.parse_args()
    dtype = torch.float64 if a.dtype == "f64" else torch.float32
    kernels = None
    if a.kernels:
        mod, cls = a.kernels.split(":")
        kernels = getattr(importlib.import_module(mod), cls)()
    obj = make_objective(th, a.intervals, a.batch, dtype, a.device)
    solver = th.HipBandedCholeskySolver if a.solver == "banded" else th.HipCholeskySolver
    opt = th.LevenbergMarquardt(obj, linear_solver_cls=solver, max_iterations=a.iters, step_size=1.0,
                                linearization_kwargs=dict(kernels=kernels) if kernels else None)
    print(f"{len(obj.cost_functions)} costs, n = {opt.linear_solver.linearization.n}, batch {a.batch}, "
          f"packed family: {type(opt.linear_solver.linearization.packed).__name__}, solver: {type(opt.linear_solver).__name__}")
    with torch.no_grad():
        info = opt.optimize(damping=0.1, track_err_history=True)
    hist = info.err_history
    print(f"objective (mean over the batch): {float(hist[:, 0].mean()):.4f} -> {float(obj.error_metric().mean()):.4f} "
          f"after {int(info.iters_done)} iterations")
    traj = torch.stack([obj.optim_vars[f"pose_{i}"].tensor for i in range(a.intervals + 1)], dim=1)   # (B, N + 1, 2)
    sdf = th.eb.SignedDistanceField2D(obj.aux_vars["sdf_origin"], obj.aux_vars["cell_size"], obj.aux_vars["sdf_data"])
    d, _ = sdf.signed_distance(traj.permute(0, 2, 1).contiguous())
    print(f"smallest clearance along the trajectories: {float(d.min()):.3f} (discs are entered where it is negative)")


if __name__ == "__main__":
    main()
