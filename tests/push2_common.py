"""The planar-pushing objective of the push2 fixtures (tests/golden/push2_f64_shared.npz, push2_f64_batched.npz, written by
tools/gen_push2_golden.py from the REAL reference), built on either API: ``th`` is ``theseus_amd`` in the tests and ``theseus`` in
the generator.  It is the objective of the reference's pose estimator (theseus/utils/examples/tactile_pose_estimation/
pose_estimator.py): SE2 object and effector poses over T time steps; costs in objective order: for every step a prior on the first
object pose (Difference, ScaleCostWeight), QuasiStaticPushingPlanar to the next step, the window of MovingFrameBetween terms
ending at the step, EffectorObjectContactPlanar and a motion-capture prior on the effector (Difference, DiagonalCostWeight).
Fixtures: B = 3, T = 6 (n = 36, 23 costs, m = 57), window min 2 / max 4 / step 1, a 12 x 16 rectangle SDF with cell size 0.25."""
import numpy as np
import torch

T = 6
WINDOW = (2, 4, 1)
FIXTURES = ("push2_f64_shared", "push2_f64_batched")
LM_KW = dict(max_iterations=5, step_size=1.0, abs_err_tolerance=0.0, rel_err_tolerance=0.0)
LM_DAMPING = 0.1
LEAVES = ("meas", "w_start", "w_qsp", "w_mfb", "w_contact", "w_mc", "sdf_data", "c_square", "eff_radius", "mocap")
F32_FACTOR, F32_FLOOR = 4.0, 16 * 2.0 ** -23   # the fp32 bound of a block: FACTOR x the reference's own fp32 distance, floored


def window_pairs(T, window=WINDOW):
    """(first step, last step) of every MovingFrameBetween term, in the estimator's order (pose_estimator.py:60-66)"""
    lo, hi, step = window
    return [(i - off, i) for i in range(lo, T) for off in range(lo, min(i, hi), step)]


def build(th, f, device="cpu", dtype=torch.float64, grad=False, T=T, window=WINDOW):
    """-> (objective, {leaf name: tensor}, [cost names in objective order]); ``grad``: the LEAVES require grad."""
    def t(key):
        return torch.from_numpy(np.asarray(f[key])).to(dtype).to(device)
    leaves = {k: t(k).clone().requires_grad_(grad) for k in LEAVES}
    obj0, eff0 = t("obj0"), t("eff0")
    objs = [th.SE2(tensor=obj0[:, i].clone(), name=f"obj_pose_{i}") for i in range(T)]
    effs = [th.SE2(tensor=eff0[:, i].clone(), name=f"eff_pose_{i}") for i in range(T)]
    start = th.SE2(tensor=t("obj_start"), name="obj_start_pose")
    mocap = [th.SE2(tensor=leaves["mocap"][:, i], name=f"motion_capture_{i}") for i in range(T)]
    pairs = window_pairs(T, window)
    meas = [th.SE2(tensor=leaves["meas"][:, k], name=f"nn_measurement_{a}_{b}") for k, (a, b) in enumerate(pairs)]
    origin = th.Point2(tensor=t("sdf_origin"), name="sdf_origin")
    cell = th.Variable(t("cell_size"), name="sdf_cell_size")
    sdf = th.Variable(leaves["sdf_data"], name="sdf_data")
    radius = th.Variable(leaves["eff_radius"], name="eff_radius")
    c_square = th.Variable(leaves["c_square"], name="c_square")
    w_start = th.ScaleCostWeight(th.Variable(leaves["w_start"], name="w_start"))
    w_qsp = th.DiagonalCostWeight(th.Variable(leaves["w_qsp"], name="qsp_weight"))
    w_mfb = th.DiagonalCostWeight(th.Variable(leaves["w_mfb"], name="mf_between_weight"))
    w_contact = th.ScaleCostWeight(th.Variable(leaves["w_contact"], name="intersect_weight"))
    w_mc = th.DiagonalCostWeight(th.Variable(leaves["w_mc"], name="mc_weight"))
    obj = th.Objective(dtype=dtype)
    k = 0
    for i in range(T):
        if i == 0:
            obj.add(th.Difference(objs[0], start, w_start, name="obj_priors_0"))
        if i < T - 1:
            obj.add(th.eb.QuasiStaticPushingPlanar(objs[i], objs[i + 1], effs[i], effs[i + 1], c_square, w_qsp, name=f"qsp_{i}"))
        while k < len(pairs) and pairs[k][1] == i:
            a = pairs[k][0]
            obj.add(th.eb.MovingFrameBetween(objs[a], objs[i], effs[a], effs[i], meas[k], w_mfb, name=f"mf_between_{a}_{i}"))
            k += 1
        obj.add(th.eb.EffectorObjectContactPlanar(objs[i], effs[i], origin, sdf, cell, radius, w_contact, name=f"intersect_{i}"))
        obj.add(th.Difference(effs[i], mocap[i], w_mc, name=f"eff_priors_{i}"))
    return obj, leaves, list(obj.cost_functions.keys())


def state_of(values, names):
    """{variable name: (B, 4)} -> (B, 4 V) in ``names`` order"""
    return torch.cat([values[k] for k in names], dim=1)


def rect_sdf(origin, cell, rows, cols, half):
    """Analytic signed distance of the axis-aligned rectangle |x| <= half[0], |y| <= half[1] on the grid: (rows, cols); x along
    the columns."""
    xs = origin[0] + cell * np.arange(cols)
    ys = origin[1] + cell * np.arange(rows)
    X, Y = np.meshgrid(xs, ys)
    qx, qy = np.abs(X) - half[0], np.abs(Y) - half[1]
    return np.hypot(np.maximum(qx, 0), np.maximum(qy, 0)) + np.minimum(np.maximum(qx, qy), 0)


def pose(x, y, theta):
    return np.array([x, y, np.cos(theta), np.sin(theta)])


def contact_cells(f):
    """(col, row) cell coordinates (B, T) of every effector in its object's frame, in transform_to's operation order -- exact
    where the object's rotation is exactly the identity and the coordinates are multiples of the cell size."""
    o, e, org, c = (np.asarray(f[k]) for k in ("obj0", "eff0", "sdf_origin", "cell_size"))
    tx, ty = e[..., 0] - o[..., 0], e[..., 1] - o[..., 1]
    ns = -o[..., 3]
    px, py = o[..., 2] * tx - ns * ty, ns * tx + o[..., 2] * ty
    return (px - org[:, None, 0]) / c, (py - org[:, None, 1]) / c


def classify(f):
    """The cases the fixture's INITIAL contact points cover: a set of names."""
    R, C = np.asarray(f["sdf_data"]).shape[1:]
    col, row = contact_cells(f)
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


def random_problem(B, T, seed, window=WINDOW, outside=0.1):
    """A second shape for the kernels alone (no reference run): random pushing trajectories, per-problem grids / weights /
    measurements; a fraction ``outside`` of the effectors lies outside the grid of its object, every contact point at least 1e-3
    cells away from a grid line."""
    rng = np.random.default_rng(seed)
    R, C, cell = 12, 16, 0.25
    origin = np.array([[-2.0, -1.5]])
    sdf = np.stack([rect_sdf(origin[0], cell, R, C, (rng.uniform(0.5, 0.9), rng.uniform(0.3, 0.6))) for _ in range(B)])
    th_o = np.cumsum(rng.normal(0, 0.15, (B, T)), axis=1) + rng.uniform(-np.pi, np.pi, (B, 1))
    t_o = np.cumsum(rng.normal(0, 0.1, (B, T, 2)), axis=1)
    out = rng.random((B, T)) < outside
    colf = np.where(out, rng.choice([-2, -1, C - 1, C], (B, T)), rng.integers(0, C - 1, (B, T))) + rng.uniform(1e-3, 1 - 1e-3, (B, T))
    rowf = np.where(out, rng.choice([-2, -1, R - 1, R], (B, T)), rng.integers(0, R - 1, (B, T))) + rng.uniform(1e-3, 1 - 1e-3, (B, T))
    qx, qy = origin[0, 0] + cell * colf, origin[0, 1] + cell * rowf
    c, s = np.cos(th_o), np.sin(th_o)
    ex, ey = t_o[..., 0] + c * qx - s * qy, t_o[..., 1] + s * qx + c * qy
    th_e = rng.uniform(-np.pi, np.pi, (B, T))
    obj0 = np.stack([t_o[..., 0], t_o[..., 1], c, s], axis=-1)
    eff0 = np.stack([ex, ey, np.cos(th_e), np.sin(th_e)], axis=-1)
    M = len(window_pairs(T, window))
    rnd_pose = lambda *shape: np.stack([pose(*v) for v in rng.normal(0, 0.3, (int(np.prod(shape)), 3))]).reshape(*shape, 4)  # noqa: E731
    mocap = eff0.copy()
    mocap[..., :2] += rng.normal(0, 0.05, (B, T, 2))
    start = obj0[:, 0].copy()
    start[:, :2] += rng.normal(0, 0.05, (B, 2))   # (a prior AT its target has a zero error block: no magnitude to bound against)
    return dict(obj0=obj0, eff0=eff0, obj_start=start, mocap=mocap, meas=rnd_pose(B, M), sdf_origin=origin,
                cell_size=np.array([[cell]]), sdf_data=sdf, eff_radius=rng.uniform(0.02, 0.2, (B, 1)), c_square=np.array([[0.9]]),
                w_start=np.array([[4.0]]), w_qsp=rng.uniform(0.5, 3, (B, 3)), w_mfb=np.array([[2.0, 1.5, 0.7]]),
                w_contact=rng.uniform(1, 5, (B, 1)), w_mc=np.array([[3.0, 3.0, 1.0]]))
