"""SE2 motion planning with a nonholonomic constraint (the reference's examples/se2_planning.py: MotionPlanner with pose_type=SE2,
nonholonomic_w=10, positive_vel_w=5, Levenberg-Marquardt with step_size=0.25 and damping=0.1) on theseus_amd's own API: a batch of
car-like robots crossing a map of discs.  Per step: Collision2D at the pose's translation, GPMotionModel between consecutive (SE2
pose, Vector(3) body velocity) pairs, Nonholonomic (no sideways velocity) and a HingeCost that keeps the forward velocity positive;
priors on the start pose and the two end velocities, the goal as an XYDifference; the planner's straight-line initialisation with the
start's heading.  The fused path is theseus_amd/planning_se2.py: PackedTrajectorySE2 -- thx_trajse2_eval + thx_block_assemble + the
tiled Cholesky at n = 6 (N + 1) + thx_trajse2_retract.
The map is synthetic: the analytic signed distance of a few discs sampled on a grid (no dataset file).
usage: python examples/se2_planning.py [--intervals 100] [--batch 16] [--iters 50] [--device cuda] [--dtype f64]
       (--kernels module:Class substitutes the kernel set -- the tests' CPU stand-in, for machines without a GPU)
"""
import argparse
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import theseus_amd as th  # noqa: E402

DISCS = ((-1.2, 0.6, 1.1), (1.8, -1.2, 1.0), (0.6, 2.6, 0.8))   # (cx, cy, radius)
ORIGIN, CELL, ROWS, COLS = (-5.0, -5.0), 0.078125, 128, 128
TOTAL_TIME = 10.0
SAFETY_DISTANCE, ROBOT_RADIUS = 1.5, 0.25
COLLISION_W, BOUNDARY_W, NONHOLONOMIC_W, POSITIVE_VEL_W = 20.0, 100.0, 10.0, 5.0


def disc_map(dtype, device):
    xs = ORIGIN[0] + CELL * torch.arange(COLS, dtype=dtype, device=device)
    ys = ORIGIN[1] + CELL * torch.arange(ROWS, dtype=dtype, device=device)
    Y, X = torch.meshgrid(ys, xs, indexing="ij")      # rows are y, columns are x
    return torch.stack([torch.hypot(X - cx, Y - cy) - r for cx, cy, r in DISCS]).min(dim=0).values.unsqueeze(0)


def make_objective(th, N, B, dtype, device, seed=0):
    """N intervals (N + 1 SE2 poses and Vector(3) velocities, n = 6 (N + 1) columns, 4 N + 4 costs), B problems with their own start /
    goal; the variables are created in the planner's order: pose_0, vel_0, pose_N, vel_N, pose_1, vel_1, ..."""
    gen = torch.Generator().manual_seed(seed)
    t = lambda *v: torch.tensor(v, dtype=dtype, device=device)  # noqa: E731
    start_xy = t(-4.0, -3.0) + 1.0 * (torch.rand(B, 2, generator=gen) - 0.5).to(dtype).to(device)
    goal = t(4.0, 3.0) + 1.0 * (torch.rand(B, 2, generator=gen) - 0.5).to(dtype).to(device)
    start = torch.cat([start_xy, t(0.0, -1.0).expand(B, 2)], dim=1)   # (the reference example's heading: cos 0, sin -1)
    origin = th.Point2(tensor=t(*ORIGIN).view(1, 2), name="sdf_origin")
    cell = th.Variable(t(CELL).view(1, 1), name="cell_size")
    sdf = th.Variable(disc_map(dtype, device), name="sdf_data")
    eps = th.Variable(t(SAFETY_DISTANCE + ROBOT_RADIUS).view(1, 1), name="cost_eps")
    dt = th.Variable(t(TOTAL_TIME / N).view(1, 1), name="dt")
    gp_w = th.eb.GPCostWeight(th.Variable(torch.eye(3, dtype=dtype, device=device).unsqueeze(0), name="Qc_inv"), dt)
    w_col = th.ScaleCostWeight(th.Variable(t(COLLISION_W).view(1, 1), name="collision_w"))
    w_bound = th.ScaleCostWeight(th.Variable(t(BOUNDARY_W).view(1, 1), name="boundary_w"))
    w_nh = th.ScaleCostWeight(th.Variable(t(NONHOLONOMIC_W).view(1, 1), name="nonholonomic_w"))
    w_pv = th.ScaleCostWeight(th.Variable(t(POSITIVE_VEL_W).view(1, 1), name="positive_vel_w"))
    # motion_planner.py: get_variable_values_from_straight_line -- positions on the line, the start's rotation, the average velocity
    s = torch.linspace(0, 1, N + 1, dtype=dtype, device=device).view(1, -1, 1)
    line = start_xy.unsqueeze(1) * (1 - s) + goal.unsqueeze(1) * s
    vel = torch.cat([(goal - start_xy) / TOTAL_TIME, torch.zeros(B, 1, dtype=dtype, device=device)], dim=1)
    poses = [th.SE2(tensor=torch.cat([line[:, i], start[:, 2:]], dim=1), name=f"pose_{i}") for i in range(N + 1)]
    vels = [th.Vector(tensor=vel.clone(), name=f"vel_{i}") for i in range(N + 1)]
    zero = lambda name: th.Vector(tensor=torch.zeros(1, 3, dtype=dtype, device=device), name=name)  # noqa: E731
    inf = float("inf")
    down, up = th.Variable(t(0.0, -inf, -inf).view(1, 3), name="vel_down_limit"), th.Variable(t(inf, inf, inf).view(1, 3), name="vel_up_limit")
    thr = th.Variable(t(1.0, 1.0, 1.0).view(1, 3), name="vel_threshold")
    obj = th.Objective(dtype=dtype)
    obj.add(th.Difference(poses[0], th.SE2(tensor=start, name="start"), w_bound, name="pose_0"))
    obj.add(th.Difference(vels[0], zero("zero_vel_0"), w_bound, name="vel_0"))
    obj.add(th.eb.XYDifference(poses[N], th.Point2(tensor=goal, name="goal"), w_bound, name="pose_N"))
    obj.add(th.Difference(vels[N], zero("zero_vel_N"), w_bound, name="vel_N"))
    for i in range(1, N + 1):
        obj.add(th.eb.Collision2D(poses[i], origin, sdf, cell, eps, w_col, name=f"collision_{i}"))
        obj.add(th.eb.GPMotionModel(poses[i - 1], vels[i - 1], poses[i], vels[i], dt, gp_w, name=f"gp_{i}"))
        obj.add(th.eb.Nonholonomic(poses[i], vels[i], w_nh, name=f"nonholonomic_{i}"))
        obj.add(th.eb.HingeCost(vels[i - 1], down, up, thr, w_pv, name=f"positive_vel_{i}"))
    return obj


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--intervals", type=int, default=100)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50)
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
    opt = th.LevenbergMarquardt(obj, linear_solver_cls=solver, max_iterations=a.iters, step_size=0.25,
                                linearization_kwargs=dict(kernels=kernels) if kernels else None)
    print(f"{len(obj.cost_functions)} costs, n = {opt.linear_solver.linearization.n}, batch {a.batch}, "
          f"packed family: {type(opt.linear_solver.linearization.packed).__name__}, solver: {type(opt.linear_solver).__name__}")
    sideways = lambda: max(float(obj.optim_vars[f"vel_{i}"].tensor[:, 1].abs().max()) for i in range(1, a.intervals + 1))  # noqa: E731
    before = sideways()
    with torch.no_grad():
        info = opt.optimize(damping=0.1, track_err_history=True)
    hist = info.err_history
    print(f"objective (mean over the batch): {float(hist[:, 0].mean()):.4f} -> {float(obj.error_metric().mean()):.4f} "
          f"after {int(info.iters_done)} iterations")
    print(f"largest |vel_y| in the body frame (the nonholonomic residual): {before:.4f} -> {sideways():.4f}")
    forward = min(float(obj.optim_vars[f"vel_{i}"].tensor[:, 0].min()) for i in range(a.intervals))
    print(f"smallest forward velocity: {forward:.4f}")


if __name__ == "__main__":
    main()
