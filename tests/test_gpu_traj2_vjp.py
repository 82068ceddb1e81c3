"""-m gpu: the fused backward of the 2D planner's implicit step (csrc/traj_kernels.hip: thx_traj2_vjp; theseus_amd/term_table.py:
TermTable.assemble(graph=True)) against the torch path of the same packed class (``fused_backward = False``) evaluated in fp64.
CPU twin: tests/test_traj2_vjp_host.py."""
import functools

import numpy as np
import pytest
import torch

from tests.helpers import load_golden
from tests.test_traj2_host import _lm, check_implicit_gradients
from tests.traj2_common import FIXTURES

pytestmark = pytest.mark.gpu
DEV = "cuda"
R, C = 6, 7
# (col, row) in cells: two active poses in one cell, one with d > eps, one left of the grid, one exactly on the last row, one exactly
# on the last column -- there the clamped corners coincide
CELLS = ((3.3, 2.4), (3.6, 2.55), (0.3, 4.6), (-0.7, 2.5), (2.3, R - 1.0), (C - 1.0, 1.4))
LEAVES = ("sdf_data", "sdf_origin", "cell_size", "cost_eps", "w_collision", "dt", "Qc_inv", "start", "goal", "w_scale", "w_diag")


def problem(B, layout, cells=CELLS, seed=3):
    """fp64 arrays of a trajectory through ``cells`` (jittered per problem by less than 0.15 cells where a pose is not meant to sit on
    a grid line); origins and cell sizes are dyadic, so a pose on a grid line is there in fp32 as well.  d = 0.25 (|cell - (3, 2)| -
    1.2) + noise below 0.01: eps = 0.55 is at least 0.05 away from every d."""
    rng = np.random.default_rng(seed)
    A = 1 if layout == "shared" else B
    cc, rr = np.meshgrid(np.arange(C), np.arange(R))
    f = dict(sdf_data=0.25 * (np.hypot(cc - 3.0, rr - 2.0) - 1.2) + rng.uniform(-0.01, 0.01, (A, R, C)),
             sdf_origin=np.array([[-0.5, -0.25]]) + 0.25 * rng.integers(0, 3, (A, 2)), cell_size=0.25 * rng.integers(1, 3, (A, 1)),
             cost_eps=np.full((A, 1), 0.55), w_collision=rng.uniform(1, 4, (A, 1)), dt=rng.uniform(0.4, 0.6, (A, 1)),
             Qc_inv=np.array([[[2.0, 0.3], [0.1, 1.5]]]) * rng.uniform(0.8, 1.2, (A, 1, 1)), w_scale=rng.uniform(2, 5, (A, 1)),
             w_diag=rng.uniform(2, 5, (A, 2)), zero=np.zeros((1, 2)))
    cell = np.asarray(cells, np.float64)[None].repeat(B, 0)                       # (B, P, 2)
    jitter = rng.uniform(-0.15, 0.15, cell.shape) * (cell != np.round(cell))
    f["poses0"] = f["sdf_origin"][:, None] + f["cell_size"][:, None] * (cell + jitter)
    f["vels0"] = rng.normal(0, 0.5, cell.shape)
    f["start"], f["goal"] = f["poses0"][:A, 0] + 0.05, f["poses0"][:A, -1] - 0.05
    f["u"] = rng.normal(0, 1, (B, 4 * cell.shape[1]))
    return f


def build(th, f, dtype, layout, gp=True):
    """-> (objective, {name: the leaf that requires grad}, the target that does not)"""
    def t(key):
        return torch.from_numpy(f[key].astype(np.float32 if dtype == torch.float32 else np.float64)).to(dtype).to(DEV)
    leaves, aux = {}, {}
    for k in LEAVES:
        if layout == "sliced":   # the auxiliary is big[:, 1]: dense per problem, read through the parent's batch stride
            leaves[k] = torch.stack([t(k) - 7, t(k), t(k) + 7], dim=1).requires_grad_(True)
            aux[k] = leaves[k][:, 1]
        else:
            leaves[k] = aux[k] = t(k).requires_grad_(True)
    P = f["poses0"].shape[1]
    poses = [th.Point2(tensor=t("poses0")[:, i].clone(), name=f"pose_{i}") for i in range(P)]
    vels = [th.Vector(tensor=t("vels0")[:, i].clone(), name=f"vel_{i}") for i in range(P)]
    v = {k: th.Variable(aux[k], name=k) for k in LEAVES if k not in ("sdf_origin", "start", "goal")}
    origin, zero = th.Point2(tensor=aux["sdf_origin"], name="sdf_origin"), th.Vector(tensor=t("zero"), name="zero")
    w_col, w_scale, w_diag = th.ScaleCostWeight(v["w_collision"]), th.ScaleCostWeight(v["w_scale"]), th.DiagonalCostWeight(v["w_diag"])
    gp_w = th.eb.GPCostWeight(v["Qc_inv"], v["dt"])
    obj = th.Objective(dtype=dtype)
    obj.add(th.Difference(poses[0], th.Point2(tensor=aux["start"], name="start"), w_scale, name="prior_start"))
    obj.add(th.Difference(poses[-1], th.Point2(tensor=aux["goal"], name="goal"), w_diag, name="prior_goal"))
    obj.add(th.Difference(vels[0], zero, w_diag, name="prior_vel"))
    for i in range(P):
        obj.add(th.eb.Collision2D(poses[i], origin, v["sdf_data"], v["cell_size"], v["cost_eps"], w_col, name=f"collision_{i}"))
    for i in range(P - 1 if gp else 0):
        obj.add(th.eb.GPMotionModel(poses[i], vels[i], poses[i + 1], vels[i + 1], v["dt"], gp_w, name=f"gp_{i}"))
    return obj, leaves, zero.tensor


def gradients(f, dtype, layout, fused, gp=True):
    """{leaf: d (g * u).sum() / d leaf as fp64 numpy} of ``packed.assemble(H, g, graph=True)``; fp32 inputs are f rounded to fp32"""
    import theseus_amd as th
    f = {k: a.astype(np.float32).astype(np.float64) for k, a in f.items()}
    obj, leaves, zero = build(th, f, dtype, layout, gp)
    lin = th.HipLinearization(obj)
    assert type(lin.packed).__name__ == "PackedTrajectory2D" and type(lin.K).__name__ == "HipKernels"
    lin.packed.fused_backward = fused
    lin._ensure_buffers()
    g = lin.packed.assemble(lin._H, lin.g, graph=True)
    (g * torch.from_numpy(f["u"][:, :g.shape[1]]).to(dtype).to(DEV)).sum().backward()
    assert zero.grad is None
    return {k: v.grad.double().cpu().numpy() for k, v in leaves.items() if gp or k not in ("dt", "Qc_inv")}


reference = functools.lru_cache(maxsize=None)(lambda B, layout, dtype: gradients(problem(B, layout), dtype, layout, False))


def worst_ratio(got, want, bound):
    """the largest |got - want| / bound over the leaves; bound(leaf name, largest magnitude of want) -> its absolute bound"""
    worst = 0.0
    for k in want:
        scale = float(np.abs(want[k]).max())
        assert scale > 0, k
        ratio = float(np.abs(got[k] - want[k]).max()) / bound(k, scale)
        print(f"  {k}: difference / bound = {ratio:.3f}")
        worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize("layout", ["shared", "batched", "sliced"])
@pytest.mark.parametrize("B", [3, 70])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_gradients_of_every_auxiliary_tensor_match_the_torch_path(dtype, B, layout):
    """fp64: 1e-12 of each gradient's largest magnitude (the family's block bound).  fp32: 4 x the torch path's own fp32 distance from
    its fp64 value, floored at 16 * 2^-23 of the largest magnitude (the pushing family's rule)."""
    want = reference(B, layout, torch.float64)
    got = gradients(problem(B, layout), dtype, layout, True)
    if dtype == torch.float64:
        bound = lambda k, scale: 1e-12 * scale  # noqa: E731
    else:
        twin = reference(B, layout, torch.float32)
        bound = lambda k, scale: max(4 * float(np.abs(twin[k] - want[k]).max()), 16 * 2.0 ** -23 * scale)  # noqa: E731
    worst = worst_ratio(got, want, bound)
    print(f"traj2_vjp {dtype} B={B} {layout}: worst difference / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("fixture", FIXTURES)
def test_the_torch_classes_are_not_evaluated(fixture, monkeypatch):
    """implicit LM on the device with the fixture's leaves requiring grad: the reference's gradients, and no weighted_jacobians_error"""
    import theseus_amd as th

    def refuse(*a, **kw):
        raise AssertionError("a cost function was evaluated by torch although the family has a VJP kernel")
    for cls in (th.eb.Collision2D, th.eb.DoubleIntegrator, th.Difference):
        monkeypatch.setattr(cls, "weighted_jacobians_error", refuse)
    g = load_golden(fixture)
    _, opt, leaves, sol, _ = _lm(th, g, None, device=DEV, backward_mode="implicit")
    assert type(opt.linear_solver.linearization.packed).__name__ == "PackedTrajectory2D"
    check_implicit_gradients(g, leaves, sol, g["var_order"].tolist())


def test_grid_scatter_across_a_sort_chunk_boundary():
    """B = 2, 259 collision terms: 1036 (cell, value) pairs, 12 more than one sort chunk; every third pose lies in one common cell, so
    that cell's run straddles the boundary and is updated by both chunks.  fp64 bound."""
    from theseus_amd._lib import THX_TRAJ2_SORT_CHUNK
    P = THX_TRAJ2_SORT_CHUNK // 4 + 3
    cells = tuple((3.4, 2.5) if i % 3 == 0 else (0.5 + (i * 0.37) % 5.0, 0.5 + (i * 0.61) % 4.0) for i in range(P))
    f = problem(2, "shared", cells, seed=11)
    want, got = gradients(f, torch.float64, "shared", False, gp=False), gradients(f, torch.float64, "shared", True, gp=False)
    assert worst_ratio(got, want, lambda k, scale: 1e-12 * scale) <= 1.0


def test_two_backward_calls_give_the_same_bits():
    f = problem(70, "shared")
    a, b = gradients(f, torch.float32, "shared", True), gradients(f, torch.float32, "shared", True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
