"""The SE2 motion planner's objective of the trajse2 fixtures (tests/golden/trajse2_f64_shared.npz, trajse2_f64_batched.npz, written
by tools/gen_trajse2_golden.py from the REAL reference's MotionPlannerObjective(pose_type=SE2, nonholonomic_w, positive_vel_w)), built
on theseus_amd's API with the planner's names and cost order: priors pose_0 (Difference on SE2), vel_0 (Difference on Vector(3)),
pose_N (XYDifference), vel_N, all with the planner's ScaleCostWeight(100); then per step i = 1 .. N: collision_i (Collision2D on
pose_i), gp_i (GPMotionModel on pose_{i-1}, vel_{i-1}, pose_i, vel_i), nonholonomic_i (pose_i, vel_i) and positive_vel_i (HingeCost on
vel_{i-1}, limits [0, -inf, -inf] / +inf, threshold 1).  ``add_extra_hinge`` -- shared with the generator, it runs on either API --
appends one HingeCost with finite limits and a DiagonalCostWeight on vel_N.
Fixtures: B = 3, N = 5 (6 poses, 6 velocities, n = 36, 25 costs, m = 69), a 12 x 16 rectangle SDF with cell size 0.25."""
import numpy as np
import torch

from tests.push2_common import pose, rect_sdf  # noqa: F401  (shared with the generator)

N = 5
FIXTURES = ("trajse2_f64_shared", "trajse2_f64_batched")
LM_KW = dict(max_iterations=5, step_size=0.25, abs_err_tolerance=0.0, rel_err_tolerance=0.0)
LM_DAMPING = 0.1
LEAVES = ("sdf_data", "collision_w", "cost_eps", "Qc_inv", "start", "goal", "nonholonomic_w", "positive_vel_w")
BOUNDARY_W = 100.0
ALL_CASES = {"left", "right", "below", "above", "interior", "on_row", "on_col", "last_row", "last_col"}


def _tensors(f, dtype, device):
    def t(key):
        return torch.from_numpy(np.asarray(f[key])).to(dtype).to(device)
    return t


def add_extra_hinge(th, obj, f, N=N, device="cpu", dtype=torch.float64):
    """One more HingeCost, on vel_N: finite limits (xh_down, xh_up), threshold xh_thr, a 3-wide DiagonalCostWeight xh_w."""
    t = _tensors(f, dtype, device)
    w = th.DiagonalCostWeight(th.Variable(t("xh_w"), name="extra_hinge_w"))
    obj.add(th.eb.HingeCost(obj.optim_vars[f"vel_{N}"], th.Variable(t("xh_down"), name="xh_down"), th.Variable(t("xh_up"), name="xh_up"),
                            th.Variable(t("xh_thr"), name="xh_thr"), w, name="extra_hinge"))


def build(th, f, device="cpu", dtype=torch.float64, grad=False, N=N):
    """-> (objective, {leaf name: tensor}, [cost names in objective order]); ``grad``: the LEAVES require grad."""
    t = _tensors(f, dtype, device)
    leaves = {k: t(k).clone().requires_grad_(grad) for k in LEAVES}
    origin = th.Point2(tensor=t("sdf_origin"), name="sdf_origin")
    start, goal = th.SE2(tensor=leaves["start"], name="start"), th.Point2(tensor=leaves["goal"], name="goal")
    cell = th.Variable(t("cell_size"), name="cell_size")
    sdf = th.Variable(leaves["sdf_data"], name="sdf_data")
    eps = th.Variable(leaves["cost_eps"], name="cost_eps")
    dt = th.Variable(t("dt"), name="dt")
    gp_w = th.eb.GPCostWeight(th.Variable(leaves["Qc_inv"], name="Qc_inv"), dt)
    col_w = th.ScaleCostWeight(th.Variable(leaves["collision_w"], name="collision_w"))
    boundary = th.ScaleCostWeight(torch.tensor(BOUNDARY_W, dtype=dtype, device=device))
    nhw = th.ScaleCostWeight(th.Variable(leaves["nonholonomic_w"], name="nonholonomic_w"))
    pvw = th.ScaleCostWeight(th.Variable(leaves["positive_vel_w"], name="positive_vel_w"))
    p0, v0 = t("pose0"), t("vel0")
    poses = [th.SE2(tensor=p0[:, i].clone(), name=f"pose_{i}") for i in range(N + 1)]
    vels = [th.Vector(tensor=v0[:, i].clone(), name=f"vel_{i}") for i in range(N + 1)]
    zeros = lambda: th.Vector(tensor=torch.zeros(1, 3, dtype=dtype, device=device))  # noqa: E731
    inf = float("inf")
    obj = th.Objective(dtype=dtype)
    obj.add(th.Difference(poses[0], start, boundary, name="pose_0"))
    obj.add(th.Difference(vels[0], zeros(), boundary, name="vel_0"))
    obj.add(th.eb.XYDifference(poses[N], goal, boundary, name="pose_N"))
    obj.add(th.Difference(vels[N], zeros(), boundary, name="vel_N"))
    for i in range(1, N + 1):
        obj.add(th.eb.Collision2D(poses[i], origin, sdf, cell, eps, col_w, name=f"collision_{i}"))
        obj.add(th.eb.GPMotionModel(poses[i - 1], vels[i - 1], poses[i], vels[i], dt, gp_w, name=f"gp_{i}"))
        obj.add(th.eb.Nonholonomic(poses[i], vels[i], nhw, name=f"nonholonomic_{i}"))
        obj.add(th.eb.HingeCost(vels[i - 1], torch.tensor([[0.0, -inf, -inf]], dtype=dtype, device=device),
                                torch.tensor([[inf, inf, inf]], dtype=dtype, device=device), 1.0, pvw, name=f"positive_vel_{i}"))
    add_extra_hinge(th, obj, f, N, device, dtype)
    return obj, leaves, list(obj.cost_functions.keys())


def state_of(values, names):
    """{variable name: (B, 4 | 3)} -> (B, 4 * poses + 3 * velocities) in ``names`` order"""
    return torch.cat([values[k] for k in names], dim=1)


def pose_cells(f):
    """(col, row) cell coordinates (B, N + 1) of every pose's translation -- exact where they are multiples of the cell size"""
    p, o, c = np.asarray(f["pose0"]), np.asarray(f["sdf_origin"]), np.asarray(f["cell_size"])
    return (p[..., 0] - o[:, None, 0]) / c, (p[..., 1] - o[:, None, 1]) / c


def classify(f):
    """The cases the fixture's INITIAL poses 1 .. N (the ones with a collision cost) cover: a set of names."""
    R, C = np.asarray(f["sdf_data"]).shape[1:]
    col, row = (v[:, 1:] for v in pose_cells(f))
    out = set()
    for name, m in (("left", col < 0), ("right", col > C - 1), ("below", row < 0), ("above", row > R - 1)):
        if m.any():
            out.add(name)
    inside = (col >= 0) & (col <= C - 1) & (row >= 0) & (row <= R - 1)
    frac = lambda v: v != np.floor(v)  # noqa: E731
    if (inside & frac(col) & frac(row)).any():
        out.add("interior")
    if (inside & ~frac(row) & frac(col) & (row < R - 1)).any():
        out.add("on_row")
    if (inside & ~frac(col) & frac(row) & (col < C - 1)).any():
        out.add("on_col")
    if (inside & (row == R - 1)).any():
        out.add("last_row")
    if (inside & (col == C - 1)).any():
        out.add("last_col")
    return out


def random_problem(B, N, seed, outside=0.1):
    """A second shape for the kernels alone (no reference run): random trajectories over and around per-problem grids; a fraction
    ``outside`` of the poses lies outside the grid, every translation at least 1e-3 cells away from a grid line, every forward
    velocity at least 1e-3 away from the hinge's bound, per-problem cost_eps / dt / Qc_inv / weights."""
    rng = np.random.default_rng(seed)
    R, C, cell = 12, 16, 0.25
    origin = np.array([[-2.0, -1.5]])
    sdf = np.stack([rect_sdf(origin[0], cell, R, C, (rng.uniform(0.5, 0.9), rng.uniform(0.3, 0.6))) for _ in range(B)])
    out = rng.random((B, N + 1)) < outside
    colf = np.where(out, rng.choice([-2, -1, C - 1, C], (B, N + 1)), rng.integers(0, C - 1, (B, N + 1))) + rng.uniform(1e-3, 1 - 1e-3, (B, N + 1))
    rowf = np.where(out, rng.choice([-2, -1, R - 1, R], (B, N + 1)), rng.integers(0, R - 1, (B, N + 1))) + rng.uniform(1e-3, 1 - 1e-3, (B, N + 1))
    theta = np.cumsum(rng.normal(0, 0.3, (B, N + 1)), axis=1) + rng.uniform(-np.pi, np.pi, (B, 1))
    pose0 = np.stack([origin[0, 0] + cell * colf, origin[0, 1] + cell * rowf, np.cos(theta), np.sin(theta)], axis=-1)
    vel0 = rng.normal(0, 0.8, (B, N + 1, 3))
    vel0[..., 0] = 1.0 + rng.choice([-1.0, 1.0], (B, N + 1)) * rng.uniform(1e-3, 1.5, (B, N + 1))
    A = rng.normal(0, 0.3, (B, 3, 3))
    start = pose0[:, 0].copy()
    start[:, :2] += rng.normal(0, 0.05, (B, 2))   # (a prior AT its target has a zero error block: no magnitude to bound against)
    return dict(pose0=pose0, vel0=vel0, start=start, goal=pose0[:, -1, :2] + rng.normal(0, 0.05, (B, 2)), sdf_origin=origin,
                cell_size=np.array([[cell]]), sdf_data=sdf, cost_eps=rng.uniform(0.2, 0.6, (B, 1)), dt=rng.uniform(0.3, 0.8, (B, 1)),
                Qc_inv=np.eye(3) * rng.uniform(0.5, 2.0, (B, 1, 1)) + A @ A.transpose(0, 2, 1), collision_w=rng.uniform(1, 6, (B, 1)),
                nonholonomic_w=np.array([[10.0]]), positive_vel_w=rng.uniform(2, 8, (B, 1)), xh_down=np.array([[-1.0, -0.5, -0.8]]),
                xh_up=np.array([[1.5, 0.5, 0.8]]), xh_thr=np.array([[0.1, 0.1, 0.1]]), xh_w=rng.uniform(0.5, 3, (B, 3)))
