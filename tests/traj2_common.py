"""The 2D motion-planning objective of the traj2 fixtures (tests/golden/traj2_f64_shared.npz, traj2_f64_batched.npz, written by
tools/gen_traj2_golden.py from the REAL reference), built on either API: ``th`` is ``theseus_amd`` in the tests and ``theseus`` in
the generator.  B = 3 problems, N = 6 intervals (7 Point2 poses, 7 Vector(2) velocities, n = 28), a 12 x 16 SDF grid with cell size
0.25; costs in objective order: start / goal priors on pose and velocity (Difference: Scale on the poses, Diagonal on the
velocities), Collision2D on every pose, GPMotionModel on every interval."""
import numpy as np
import torch

N = 6
FIXTURES = ("traj2_f64_shared", "traj2_f64_batched")
LM_KW = dict(max_iterations=5, step_size=1.0, abs_err_tolerance=0.0, rel_err_tolerance=0.0)
LM_DAMPING = 0.1
LEAVES = ("sdf_data", "cost_eps", "Qc_inv", "start", "goal")


def build(th, f, device="cpu", dtype=torch.float64, grad=False, N=N, prefix=""):
    """-> (objective, {leaf name: tensor}, [cost names in objective order]); ``grad``: the LEAVES require grad."""
    def t(key):
        return torch.from_numpy(np.asarray(f[key])).to(dtype).to(device)
    leaves = {k: t(k).clone().requires_grad_(grad) for k in LEAVES}
    origin = th.Point2(tensor=t("sdf_origin"), name="sdf_origin")
    cell = th.Variable(t("cell_size"), name="cell_size")
    sdf = th.Variable(leaves["sdf_data"], name="sdf_data")
    eps = th.Variable(leaves["cost_eps"], name="cost_eps")
    dt = th.Variable(t("dt"), name="dt")
    gp_w = th.eb.GPCostWeight(th.Variable(leaves["Qc_inv"], name="Qc_inv"), dt)
    w_col = th.ScaleCostWeight(th.Variable(t("w_collision"), name="w_collision"))
    w_pose = th.ScaleCostWeight(th.Variable(t("w_pose"), name="w_pose"))
    w_vel = th.DiagonalCostWeight(th.Variable(t("w_vel"), name="w_vel"))
    p0, v0 = t("poses0"), t("vels0")
    poses = [th.Point2(tensor=p0[:, i].clone(), name=f"pose_{i}") for i in range(N + 1)]
    vels = [th.Vector(tensor=v0[:, i].clone(), name=f"vel_{i}") for i in range(N + 1)]
    zero = th.Vector(tensor=torch.zeros(1, 2, dtype=dtype, device=device), name="zero_vel")
    obj = th.Objective(dtype=dtype)
    obj.add(th.Difference(poses[0], th.Point2(tensor=leaves["start"], name="start"), w_pose, name="prior_start"))
    obj.add(th.Difference(vels[0], zero, w_vel, name="prior_start_vel"))
    obj.add(th.Difference(poses[N], th.Point2(tensor=leaves["goal"], name="goal"), w_pose, name="prior_goal"))
    obj.add(th.Difference(vels[N], zero, w_vel, name="prior_goal_vel"))
    for i in range(N + 1):
        obj.add(th.eb.Collision2D(poses[i], origin, sdf, cell, eps, w_col, name=f"collision_{i}"))
    for i in range(N):
        obj.add(th.eb.GPMotionModel(poses[i], vels[i], poses[i + 1], vels[i + 1], dt, gp_w, name=f"gp_{i}"))
    return obj, leaves, list(obj.cost_functions.keys())


def slice_aux(obj, f, device="cpu", dtype=torch.float64):
    """Replace three auxiliaries of ``obj`` (built from ``f``) by views into larger tensors: one problem's values are dense, the
    batch stride is not their width -- cost_eps a (B, 1) column of a (B, 3) tensor, the start target a (B, 2) column range of a
    (B, 5) tensor, sdf_data ``big[:, 0]`` of a (B, 2, R, C) tensor; the rest of the parents holds values no cost should ever see.
    -> {name: parent tensor}"""
    B = f["poses0"].shape[0]

    def parent(key, shape, index):
        big = torch.full(shape, -7.0, dtype=dtype, device=device)
        big[index] = torch.from_numpy(np.asarray(f[key])).to(dtype).to(device)   # (a shared (1, ...) value is broadcast)
        obj.get_variable(key).tensor = big[index]
        assert obj.get_variable(key).tensor.shape[0] == B and not big[index].is_contiguous() and big[index][0].is_contiguous()
        return big
    R, C = f["sdf_data"].shape[1:]
    s = slice(None)
    return {"cost_eps": parent("cost_eps", (B, 3), (s, slice(1, 2))), "start": parent("start", (B, 5), (s, slice(2, 4))),
            "sdf_data": parent("sdf_data", (B, 2, R, C), (s, 0))}


def state_of(values, names):
    """{variable name: (B, 2)} -> (B, n) in ``names`` order"""
    return torch.cat([values[k] for k in names], dim=1)


def disc_sdf(origin, cell, rows, cols, discs):
    """Analytic signed distance of a union of discs ((cx, cy, r), ...) on the grid: (rows, cols); x along the columns."""
    xs = origin[0] + cell * np.arange(cols)
    ys = origin[1] + cell * np.arange(rows)
    X, Y = np.meshgrid(xs, ys)
    return np.min([np.hypot(X - cx, Y - cy) - r for cx, cy, r in discs], axis=0)


def classify(f):
    """The cases the fixture's INITIAL points cover, by exact arithmetic on the fp64 inputs (cell size and origins are multiples of
    0.25): a set of names."""
    p, o, c = np.asarray(f["poses0"]), np.asarray(f["sdf_origin"]), np.asarray(f["cell_size"])
    R, C = np.asarray(f["sdf_data"]).shape[1:]
    col, row = (p[..., 0] - o[:, None, 0]) / c, (p[..., 1] - o[:, None, 1]) / c
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


ALL_CASES = {"left", "right", "below", "above", "interior", "on_row", "on_col", "last_row", "last_col"}


def random_problem(B, N, seed, dtype=np.float64):
    """A second shape for the kernels alone (no reference run): random trajectories over and around the grid, per-problem grids."""
    rng = np.random.default_rng(seed)
    R, C, cell = 12, 16, 0.25
    origin = np.array([[-2.0, -1.5]])
    sdf = np.stack([disc_sdf(origin[0], cell, R, C, [(rng.uniform(-1.5, 1.2), rng.uniform(-1, 0.8), rng.uniform(0.2, 0.6)),
                                                       (rng.uniform(-1.5, 1.2), rng.uniform(-1, 0.8), rng.uniform(0.2, 0.6))])
                    for _ in range(B)])
    # cell coordinates at least 1e-3 away from every grid line, a tenth of the points outside the grid
    colf = rng.integers(-2, C + 1, (B, N + 1)) + rng.uniform(1e-3, 1 - 1e-3, (B, N + 1))
    rowf = rng.integers(-2, R + 1, (B, N + 1)) + rng.uniform(1e-3, 1 - 1e-3, (B, N + 1))
    poses0 = np.stack([origin[0, 0] + cell * colf, origin[0, 1] + cell * rowf], axis=-1)
    return dict(sdf_origin=origin, cell_size=np.array([[cell]]), sdf_data=sdf, cost_eps=np.array([[0.4]]), dt=np.array([[0.5]]),
                Qc_inv=np.array([[[2.0, 0.3], [0.3, 1.5]]]) * rng.uniform(0.5, 2.0, (B, 1, 1)), w_collision=rng.uniform(1, 6, (B, 1)),
                w_pose=np.array([[10.0]]), w_vel=np.array([[3.0, 5.0]]), start=poses0[:, 0] + 0.05, goal=poses0[:, -1] - 0.05,
                poses0=poses0, vels0=rng.normal(0, 0.5, (B, N + 1, 2)))
