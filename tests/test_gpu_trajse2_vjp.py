"""-m gpu: the fused backward of the SE2 planner's implicit step (csrc/trajse2_vjp_kernels.hip: thx_trajse2_vjp; theseus_amd/
planning_se2.py: PackedTrajectorySE2.assemble(graph=True)) against the torch path of the same packed class (``fused_backward = False``)
evaluated in fp64.  CPU twin: tests/test_trajse2_vjp_host.py."""
import functools

import numpy as np
import pytest
import torch

from tests.helpers import load_golden
from tests.push2_common import F32_FACTOR, F32_FLOOR
from tests.test_gpu_push2_vjp import bilinear
from tests.test_gpu_traj2_vjp import worst_ratio
from tests.test_push2_host import check_implicit_gradients
from tests.test_trajse2_host import _lm
from tests.trajse2_common import FIXTURES, N, pose_cells, random_problem

pytestmark = pytest.mark.gpu
DEV = "cuda"
AUX = ("sdf_data", "sdf_origin", "cell_size", "cost_eps", "collision_w", "nonholonomic_w", "positive_vel_w", "xh_w", "w_start", "w_vel",
       "w_goal", "dt", "dt_w", "Qc_inv", "start", "goal", "vel_target", "pv_down", "pv_up", "pv_thr", "xh_down", "xh_up", "xh_thr")
ON_LINE = {(0, 1): (3.0, 2.5), (1, 2): (4.4, 11.0)}   # (problem, pose) -> (col, row): on a column line, on the last row (R = 12)
OUTSIDE = (-1.5, 2.5)
AT_BOUND = (0, 0)   # (problem, velocity): its forward component is exactly down + thr = 1: the comparison is strict, a zero record


def objective(th, f, dtype, layout, device=DEV):
    """-> (objective, {name: the leaf that requires grad}): every auxiliary tensor is a leaf.  The planner's costs (tests/
    trajse2_common.py) plus the extra finite-limit hinge and one more prior of each kind with the other weight width."""
    def t(key):
        return torch.from_numpy(f[key].astype(np.float32 if dtype == torch.float32 else np.float64)).to(dtype).to(device)
    leaves, aux = {}, {}
    for k in AUX:
        if layout == "sliced":   # the auxiliary is big[:, 1]: dense per problem, read through the parent's batch stride
            leaves[k] = torch.stack([t(k) - 7, t(k), t(k) + 7], dim=1).requires_grad_(True)
            aux[k] = leaves[k][:, 1]
        else:
            leaves[k] = aux[k] = t(k).requires_grad_(True)
    v = {k: th.Variable(aux[k], name=k) for k in AUX}
    scale, diag = (lambda k: th.ScaleCostWeight(v[k])), (lambda k: th.DiagonalCostWeight(v[k]))
    origin, goal = th.Point2(tensor=aux["sdf_origin"], name="origin"), th.Point2(tensor=aux["goal"], name="goal_xy")
    start, vel_target = th.SE2(tensor=aux["start"], name="start_pose"), th.Vector(tensor=aux["vel_target"], name="vel_t")
    gp_w = th.eb.GPCostWeight(v["Qc_inv"], v["dt_w"])
    poses = [th.SE2(tensor=t("pose0")[:, i].clone(), name=f"pose_{i}") for i in range(N + 1)]
    vels = [th.Vector(tensor=t("vel0")[:, i].clone(), name=f"vel_{i}") for i in range(N + 1)]
    obj = th.Objective(dtype=dtype)
    obj.add(th.Difference(poses[0], start, scale("w_start"), name="pose_0"))
    obj.add(th.Difference(vels[0], vel_target, diag("w_vel"), name="vel_0"))
    obj.add(th.eb.XYDifference(poses[N], goal, diag("w_goal"), name="pose_N"))
    obj.add(th.Difference(vels[N], vel_target, scale("w_start"), name="vel_N"))
    obj.add(th.Difference(poses[N], start, diag("w_vel"), name="pose_N_se2"))
    obj.add(th.eb.XYDifference(poses[0], goal, scale("w_start"), name="pose_0_xy"))
    for i in range(1, N + 1):
        obj.add(th.eb.Collision2D(poses[i], origin, v["sdf_data"], v["cell_size"], v["cost_eps"], scale("collision_w"), name=f"collision_{i}"))
        obj.add(th.eb.GPMotionModel(poses[i - 1], vels[i - 1], poses[i], vels[i], v["dt"], gp_w, name=f"gp_{i}"))
        obj.add(th.eb.Nonholonomic(poses[i], vels[i], scale("nonholonomic_w"), name=f"nonholonomic_{i}"))
        obj.add(th.eb.HingeCost(vels[i - 1], v["pv_down"], v["pv_up"], v["pv_thr"], scale("positive_vel_w"), name=f"positive_vel_{i}"))
    obj.add(th.eb.HingeCost(vels[N], v["xh_down"], v["xh_up"], v["xh_thr"], diag("xh_w"), name="extra_hinge"))
    return obj, leaves


def assert_well_defined(f, layout):
    """with the torch classes on the CPU in fp64: the reference has no kink within reach of an fp32 rounding"""
    import theseus_amd as th
    from theseus_amd.kernels import se2_eps
    switches = [x for d in (torch.float32, torch.float64) for x in (se2_eps(d).near_zero, se2_eps(d).d_near_zero)]
    obj, _ = objective(th, f, torch.float64, layout, "cpu")
    R, C = f["sdf_data"].shape[-2:]
    col, row = (a[:, 1:].copy() for a in pose_cells(f))   # (the poses with a collision cost)
    away = np.minimum(np.abs(col - np.round(col)), np.abs(row - np.round(row)))
    for (b, i), (c, r) in ON_LINE.items():
        assert (col[b, i - 1], row[b, i - 1]) == (c, r)
        away[b, i - 1] = 1.0
    outside = (col < 0) | (col > C - 1) | (row < 0) | (row > R - 1)
    assert away.min() >= 1e-3 and outside.any()
    active = []
    with torch.no_grad():
        for name, c in obj.cost_functions.items():
            kind = type(c).__name__
            if kind == "Collision2D":
                gap = c.cost_eps.tensor.view(-1, 1) - c._distances()[0]
                assert float(gap.abs().min()) >= 0.02, name
                active.append((gap > 0).view(-1).numpy() & ~outside[:, int(name.split("_")[1]) - 1])
            elif kind == "HingeCost":
                val, thr = c.vector.tensor, c.threshold.tensor
                near = torch.minimum((val - (c.down_limit.tensor + thr)).abs(), (val - (c.up_limit.tensor - thr)).abs()) < 1e-3
                if name == f"positive_vel_{AT_BOUND[1] + 1}":
                    assert float(val[AT_BOUND[0], 0]) == 1.0 == float((c.down_limit.tensor + thr).expand_as(val)[AT_BOUND[0], 0])
                    near[AT_BOUND[0], 0] = False
                assert not bool(near.any()), name
            elif kind in ("GPMotionModel", "Difference") and "SE2" in type(c.optim_vars()[0]).__name__:
                rot = (c._pose_diff(False)[0] if kind == "GPMotionModel" else c.jacobians()[1])[:, 2].abs()
                clear = (rot > 1e-5) & (rot < np.pi - 1e-5) & (torch.stack([(rot - x).abs() for x in switches]).amin(0) > 1e-5)
                if kind == "GPMotionModel":   # (see problem(): between the two dtypes' thresholds the reference itself is ambiguous)
                    clear &= rot > max(switches)
                assert bool(((rot == 0) | clear).all()), name   # (exactly 0 is inside the Taylor branch of both dtypes)
            if kind in ("Difference", "XYDifference"):
                assert bool((c.jacobians()[1] != 0).any(dim=1).all()), name
    active = np.stack(active, axis=1)
    assert active.any() and (~active & ~outside).any()   # a collision with d < eps, and one inside the grid with d > eps


@functools.lru_cache(maxsize=None)
def problem(B, layout, seed=3):
    """random_problem(B, 5, seed) (6 poses, 6 velocities, per-problem grids) with every auxiliary tensor shared (1, ...) or per
    problem, a Qc_inv that is not symmetric (its upper triangle moves, both triangles stay positive definite), two poses on grid
    lines, one outside the grid, one forward velocity exactly at the hinge's bound; as in tests/test_gpu_push2_vjp.py a pose whose
    distance is within 0.02 of cost_eps is moved outside the grid (origin and cell size are dyadic: exact in fp32 too).
    The rotations are drawn here: a GP pair's relative rotation is exactly 0 or above every Taylor threshold of BOTH dtypes.  Between
    the fp64 (1e-3) and the fp32 (0.1) threshold the fp64 reference differentiates the closed form of Jlog and every fp32 evaluation its
    series; on rotations rounded to fp32 (c^2 + s^2 = 1 + 1e-7) the closed form's 0.5 s / (1 - c) moves by 1e-5 relative, 3 % of
    k = 1 / th - 0.5 s / (1 - c) at th = 0.08, so the two are different functions there: with random_problem's own rotations the torch
    path in fp64 with the fp32 thresholds is 0.011 from the fp64 reference in d / d dt (of 649, B = 3, shared), five times the fp32
    torch path's distance (0.002, where rounding happens to cancel it), 11.2 of 1426 in d / d dt_w (the fp32 torch path: 11.2)."""
    f = random_problem(B, N, seed)
    # consecutive rotations differ by 0.12 ... 0.6 rad, or (the last pair of problem 0) by exactly 0
    rng = np.random.default_rng(seed + 1)
    theta = np.cumsum(rng.choice([-1.0, 1.0], (B, N + 1)) * rng.uniform(0.12, 0.6, (B, N + 1)), axis=1) + rng.uniform(-np.pi, np.pi, (B, 1))
    theta[0, N] = theta[0, N - 1]
    f["pose0"][..., 2], f["pose0"][..., 3] = np.cos(theta), np.sin(theta)
    f["start"][:, 2:] = f["pose0"][:, 0, 2:]
    f["Qc_inv"] = f["Qc_inv"] + np.array([[0.0, 0.05, -0.03], [0.0, 0.0, 0.04], [0.0, 0.0, 0.0]])
    f.update(dt_w=f["dt"] * 1.25, vel_target=f["vel0"][:, 0] * 0.1 + 0.05, w_start=f["collision_w"] + 1.0, w_vel=f["xh_w"] + 1.0,
             w_goal=f["xh_w"][:, :2] + 2.0, pv_down=np.array([[0.0, -np.inf, -np.inf]]), pv_up=np.full((1, 3), np.inf),
             pv_thr=np.ones((1, 3)))
    for k in AUX:
        f[k] = np.broadcast_to(f[k], (B,) + f[k].shape[1:])[:1 if layout == "shared" else B].copy()
    col, row = pose_cells(f)
    for (b, i), (c, r) in ON_LINE.items():
        col[b, i], row[b, i] = c, r
    col[2, 3], row[2, 3] = OUTSIDE
    near = np.abs(bilinear(f["sdf_data"], col, row) - f["cost_eps"]) < 0.02
    near[:, 0] = False   # (pose 0 has no collision cost)
    col[near], row[near] = OUTSIDE
    f["pose0"][..., 0], f["pose0"][..., 1] = f["sdf_origin"][:, :1] + f["cell_size"] * col, f["sdf_origin"][:, 1:] + f["cell_size"] * row
    f["vel0"][AT_BOUND[0], AT_BOUND[1], 0] = 1.0
    f["u"] = np.random.default_rng(seed).normal(0, 1, (B, 6 * (N + 1)))
    assert_well_defined(f, layout)
    return f


def gradients(f, dtype, layout, fused):
    """{leaf: d (g * u).sum() / d leaf as fp64 numpy} of ``packed.assemble(H, g, graph=True)``; fp32 inputs are f rounded to fp32"""
    import theseus_amd as th
    f = {k: a.astype(np.float32).astype(np.float64) for k, a in f.items()}
    obj, leaves = objective(th, f, dtype, layout)
    lin = th.HipLinearization(obj)
    assert type(lin.packed).__name__ == "PackedTrajectorySE2" and type(lin.K).__name__ == "HipKernels"
    lin.packed.fused_backward = fused
    lin._ensure_buffers()
    g = lin.packed.assemble(lin._H, lin.g, graph=True)
    assert (type(g.grad_fn).__name__ == "_FusedGradientBackward") == fused
    (g * torch.from_numpy(f["u"]).to(dtype).to(DEV)).sum().backward()
    return {k: v.grad.double().cpu().numpy() for k, v in leaves.items()}


reference = functools.lru_cache(maxsize=None)(lambda B, layout, dtype: gradients(problem(B, layout), dtype, layout, False))


@pytest.mark.parametrize("layout", ["shared", "batched", "sliced"])
@pytest.mark.parametrize("B", [3, 70])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_gradients_of_every_auxiliary_tensor_match_the_torch_path(dtype, B, layout):
    """fp64: 1e-12 of each gradient's largest magnitude.  fp32: F32_FACTOR x the torch path's own fp32 distance from its fp64 value,
    floored at F32_FLOOR of the largest magnitude.  The +inf up_limit is never exceeded: its gradient is exactly 0
    on both routes, as is that of the -inf components of the down_limit."""
    want = dict(reference(B, layout, torch.float64))
    got = gradients(problem(B, layout), dtype, layout, True)
    assert not want.pop("pv_up").any() and not got["pv_up"].any() and not got["pv_down"][..., 1:].any()
    if dtype == torch.float64:
        bound = lambda k, scale: 1e-12 * scale  # noqa: E731
    else:
        twin = reference(B, layout, torch.float32)
        bound = lambda k, scale: max(F32_FACTOR * float(np.abs(twin[k] - want[k]).max()), F32_FLOOR * scale)  # noqa: E731
    worst = worst_ratio(got, want, bound)
    print(f"trajse2_vjp {dtype} B={B} {layout}: worst difference / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("fixture", FIXTURES)
def test_the_torch_classes_are_not_evaluated(fixture, monkeypatch):
    """implicit LM on the device with the fixture's leaves requiring grad: the reference's gradients, and no weighted_jacobians_error"""
    import theseus_amd as th

    def refuse(*a, **kw):
        raise AssertionError("a cost function was evaluated by torch although the family has a VJP kernel")
    for cls in (th.eb.Collision2D, th.eb.DoubleIntegrator, th.eb.Nonholonomic, th.eb.HingeCost, th.eb.XYDifference, th.Difference):
        monkeypatch.setattr(cls, "weighted_jacobians_error", refuse)
    g = load_golden(fixture)
    _, opt, leaves, sol, _ = _lm(th, g, None, device=DEV, backward_mode="implicit")
    assert type(opt.linear_solver.linearization.packed).__name__ == "PackedTrajectorySE2"
    check_implicit_gradients(g, leaves, sol, g["var_order"].tolist())


def test_two_backward_calls_give_the_same_bits():
    f = problem(70, "shared")
    a, b = gradients(f, torch.float32, "shared", True), gradients(f, torch.float32, "shared", True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
