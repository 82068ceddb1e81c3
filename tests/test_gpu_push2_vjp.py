"""-m gpu: the fused backward of the planar-pushing implicit step (csrc/push_vjp_kernels.hip: thx_push2_vjp; theseus_amd/pushing.py:
PackedPlanarPushing.assemble(graph=True)) against the torch path of the same packed class (``fused_backward = False``) evaluated in
fp64.  CPU twin: tests/test_push2_vjp_host.py."""
import functools

import numpy as np
import pytest
import torch

from tests.helpers import load_golden
from tests.push2_common import F32_FACTOR, F32_FLOOR, FIXTURES, T, contact_cells, random_problem, window_pairs
from tests.test_gpu_traj2_vjp import worst_ratio
from tests.test_push2_host import _lm, check_implicit_gradients

pytestmark = pytest.mark.gpu
DEV = "cuda"
AUX = ("meas", "mocap", "obj_start", "sdf_data", "sdf_origin", "cell_size", "eff_radius", "c_square", "w_start", "w_qsp", "w_mfb",
       "w_contact", "w_mc")
ON_LINE = {(0, 0): (3.0, 2.5), (1, 0): (4.5, 2.0)}   # (problem, step) -> (col, row): on a column line, on a row line
OUTSIDE = (-1.5, 2.5)


def place(f, col, row):
    """put every effector at cell coordinates (col, row) (B, Te) of its object's frame"""
    o = f["obj0"]
    q = f["sdf_origin"][:, None] + f["cell_size"][:, None] * np.stack([col, row], -1)
    f["eff0"][..., 0] = o[..., 0] + o[..., 2] * q[..., 0] - o[..., 3] * q[..., 1]
    f["eff0"][..., 1] = o[..., 1] + o[..., 3] * q[..., 0] + o[..., 2] * q[..., 1]


def objective(th, f, dtype, layout, device=DEV, chain=True):
    """-> (objective, {name: the leaf that requires grad}): every auxiliary tensor is a leaf; ``chain`` False: contact costs of ONE
    object pose and priors only"""
    def t(key):
        return torch.from_numpy(f[key].astype(np.float32 if dtype == torch.float32 else np.float64)).to(dtype).to(device)
    leaves, aux = {}, {}
    for k in AUX:
        if layout == "sliced":   # the auxiliary is big[:, 1]: dense per problem, read through the parent's batch stride
            leaves[k] = torch.stack([t(k) - 7, t(k), t(k) + 7], dim=1).requires_grad_(True)
            aux[k] = leaves[k][:, 1]
        else:
            leaves[k] = aux[k] = t(k).requires_grad_(True)
    objs = [th.SE2(tensor=t("obj0")[:, i].clone(), name=f"obj_{i}") for i in range(f["obj0"].shape[1])]
    effs = [th.SE2(tensor=t("eff0")[:, i].clone(), name=f"eff_{i}") for i in range(f["eff0"].shape[1])]
    v = {k: th.Variable(aux[k], name=k) for k in AUX}
    w = {k: (th.ScaleCostWeight if f[k].shape[-1] == 1 else th.DiagonalCostWeight)(v[k]) for k in AUX if k.startswith("w_")}
    origin = th.Point2(tensor=aux["sdf_origin"], name="origin")
    obj = th.Objective(dtype=dtype)
    obj.add(th.Difference(objs[0], th.SE2(tensor=aux["obj_start"], name="start"), w["w_start"], name="prior_obj"))
    for i, e in enumerate(effs):
        o = objs[min(i, len(objs) - 1)]
        obj.add(th.eb.EffectorObjectContactPlanar(o, e, origin, v["sdf_data"], v["cell_size"], v["eff_radius"], w["w_contact"], name=f"contact_{i}"))
        if chain or i == 0:
            obj.add(th.Difference(e, th.SE2(tensor=aux["mocap"][:, i], name=f"mocap_{i}"), w["w_mc"], name=f"prior_eff_{i}"))
        if chain and i + 1 < len(effs):
            obj.add(th.eb.QuasiStaticPushingPlanar(o, objs[i + 1], e, effs[i + 1], v["c_square"], w["w_qsp"], name=f"qsp_{i}"))
    for k, (a, b) in enumerate(window_pairs(len(objs)) if chain else ()):
        obj.add(th.eb.MovingFrameBetween(objs[a], objs[b], effs[a], effs[b], th.SE2(tensor=aux["meas"][:, k], name=f"meas_{k}"),
                                         w["w_mfb"], name=f"mfb_{k}"))
    return obj, leaves


def assert_well_defined(f, layout, chain, on_line):
    """with the torch classes on the CPU in fp64: the reference has no kink within reach of an fp32 rounding"""
    import theseus_amd as th
    from theseus_amd.kernels import se2_eps
    switches = [x for d in (torch.float32, torch.float64) for x in (se2_eps(d).near_zero, se2_eps(d).d_near_zero)]
    obj, _ = objective(th, f, torch.float64, layout, "cpu", chain)
    col, row = contact_cells(dict(f, obj0=np.broadcast_to(f["obj0"], f["eff0"].shape)))
    R, C = f["sdf_data"].shape[-2:]
    away = np.minimum(np.abs(col - np.round(col)), np.abs(row - np.round(row)))
    for b, i in on_line:
        assert away[b, i] == 0 and tuple(f["obj0"][b, min(i, f["obj0"].shape[1] - 1), 2:]) == (1.0, 0.0)
        away[b, i] = 1.0
    assert away.min() >= 1e-3 and ((col < 0) | (col > C - 1) | (row < 0) | (row > R - 1)).any()
    zero_rotations = 0
    for c in obj.cost_functions.values():
        with torch.no_grad():
            if "Contact" in type(c).__name__:
                assert float((c._distances()[0] - c.eff_radius.tensor).abs().min()) >= 0.02, c.name
            elif "Quasi" not in type(c).__name__:
                rot = c.jacobians()[1][:, 2].abs()   # (Difference.error() on SE2 is a kernel)
                zero_rotations += int((rot == 0).sum()) * ("Moving" in type(c).__name__)
                clear = (rot > 1e-4) & (rot < np.pi - 1e-3) & (torch.stack([(rot - x).abs() for x in switches]).amin(0) > 1e-5)
                assert bool(((rot == 0) | clear).all()), c.name
    assert zero_rotations >= 1 or not chain


def bilinear(sdf, col, row):
    """SignedDistanceField2D.signed_distance on cell coordinates (B, P) of (B|1, R, C) grids"""
    R, C = sdf.shape[-2:]
    lr, lc = np.floor(row), np.floor(col)
    at = lambda r, c: sdf[np.arange(col.shape[0])[:, None] % sdf.shape[0], np.clip(r, 0, R - 1).astype(int), np.clip(c, 0, C - 1).astype(int)]  # noqa: E731
    d = ((lr + 1 - row) * ((lc + 1 - col) * at(lr, lc) + (col - lc) * at(lr, lc + 1))
         + (row - lr) * ((lc + 1 - col) * at(lr + 1, lc) + (col - lc) * at(lr + 1, lc + 1)))
    return np.where((col < 0) | (col > C - 1) | (row < 0) | (row > R - 1), 0.0, d)


@functools.lru_cache(maxsize=None)
def problem(B, layout, seed=7):
    """random_problem (T = 6, window (2, 4, 1): 23 costs, all four kinds, both weight widths) with every auxiliary tensor shared (1, ...)
    or per problem; the first MovingFrameBetween of problem 0 has identity rotations throughout (residual rotation exactly 0), two
    contact points sit on a grid line under an identity object rotation, and a contact point with |d - r| < 0.02 is moved outside."""
    f = random_problem(B, T, seed, outside=0.15)
    for k in AUX:
        f[k] = np.broadcast_to(f[k], (B,) + f[k].shape[1:])[:1 if layout == "shared" else B].copy()
    col, row = contact_cells(f)
    a, b = window_pairs(T)[0]
    for bb, i in [(0, a), (0, b)] + list(ON_LINE):
        f["obj0"][bb, i, 2:] = f["eff0"][bb, i, 2:] = (1.0, 0.0)
    f["meas"][0, 0, 2:] = (1.0, 0.0)
    for (bb, i), (c, r) in ON_LINE.items():
        f["obj0"][bb, i, :2] = (0.5, 0.25)
        col[bb, i], row[bb, i] = c, r
    near = np.abs(bilinear(f["sdf_data"], col, row) - f["eff_radius"]) < 0.02
    col[near], row[near] = OUTSIDE
    place(f, col, row)
    f["u"] = np.random.default_rng(seed).normal(0, 1, (B, 6 * T))
    assert_well_defined(f, layout, True, ON_LINE)
    return f


def gradients(f, dtype, layout, fused, chain=True):
    """{leaf: d (g * u).sum() / d leaf as fp64 numpy} of ``packed.assemble(H, g, graph=True)``; fp32 inputs are f rounded to fp32"""
    import theseus_amd as th
    f = {k: a.astype(np.float32).astype(np.float64) for k, a in f.items()}
    obj, leaves = objective(th, f, dtype, layout, chain=chain)
    lin = th.HipLinearization(obj)
    assert type(lin.packed).__name__ == "PackedPlanarPushing" and type(lin.K).__name__ == "HipKernels"
    lin.packed.fused_backward = fused
    lin._ensure_buffers()
    g = lin.packed.assemble(lin._H, lin.g, graph=True)
    assert (type(g.grad_fn).__name__ == "_FusedGradientBackward") == fused
    (g * torch.from_numpy(f["u"]).to(dtype).to(DEV)).sum().backward()
    return {k: v.grad.double().cpu().numpy() for k, v in leaves.items() if chain or k not in ("meas", "c_square", "w_qsp", "w_mfb")}


reference = functools.lru_cache(maxsize=None)(lambda B, layout, dtype: gradients(problem(B, layout), dtype, layout, False))


@pytest.mark.parametrize("layout", ["shared", "batched", "sliced"])
@pytest.mark.parametrize("B", [3, 70])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_gradients_of_every_auxiliary_tensor_match_the_torch_path(dtype, B, layout):
    """fp64: 1e-12 of each gradient's largest magnitude.  fp32: F32_FACTOR x the torch path's own fp32 distance from its fp64 value,
    floored at F32_FLOOR of the largest magnitude."""
    want = reference(B, layout, torch.float64)
    got = gradients(problem(B, layout), dtype, layout, True)
    if dtype == torch.float64:
        bound = lambda k, scale: 1e-12 * scale  # noqa: E731
    else:
        twin = reference(B, layout, torch.float32)
        bound = lambda k, scale: max(F32_FACTOR * float(np.abs(twin[k] - want[k]).max()), F32_FLOOR * scale)  # noqa: E731
    worst = worst_ratio(got, want, bound)
    print(f"push2_vjp {dtype} B={B} {layout}: worst difference / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("fixture", FIXTURES)
def test_the_torch_classes_are_not_evaluated(fixture, monkeypatch):
    """implicit LM on the device with the fixture's leaves requiring grad: the reference's gradients, and no weighted_jacobians_error"""
    import theseus_amd as th

    def refuse(*a, **kw):
        raise AssertionError("a cost function was evaluated by torch although the family has a VJP kernel")
    for cls in (th.eb.QuasiStaticPushingPlanar, th.eb.MovingFrameBetween, th.eb.EffectorObjectContactPlanar, th.Difference):
        monkeypatch.setattr(cls, "weighted_jacobians_error", refuse)
    g = load_golden(fixture)
    _, opt, leaves, sol, _ = _lm(th, g, None, device=DEV, backward_mode="implicit")
    assert type(opt.linear_solver.linearization.packed).__name__ == "PackedPlanarPushing"
    check_implicit_gradients(g, leaves, sol, g["var_order"].tolist())


def chunk_problem():
    """B = 2, 259 contact costs of one object pose on one shared grid: 1036 (cell, value) pairs, 12 more than one sort chunk; every
    third contact point lies in one common cell, so that cell's run straddles the boundary and is updated by both chunks."""
    from theseus_amd._lib import THX_TRAJ2_SORT_CHUNK
    P = THX_TRAJ2_SORT_CHUNK // 4 + 3
    f = random_problem(2, P, 11)
    for k in AUX:
        f[k] = f[k][:1].copy()
    f["obj0"] = f["obj0"][:, :1]
    i = np.arange(P)
    col = np.where(i % 3 == 0, 3.4, 0.535 + (i * 0.37) % 13.0) + np.array([[0.0], [0.05]])
    row = np.where(i % 3 == 0, 2.5, 0.535 + (i * 0.61) % 9.0) + np.array([[0.0], [0.05]])
    near = np.abs(bilinear(f["sdf_data"], col, row) - f["eff_radius"]) < 0.02
    assert not near[:, ::3].any()
    near[:, 1] = True
    col[near], row[near] = OUTSIDE
    place(f, col, row)
    f["u"] = np.random.default_rng(11).normal(0, 1, (2, 3 * (P + 1)))
    assert_well_defined(f, "shared", False, ())
    return f


def test_grid_scatter_across_a_sort_chunk_boundary():
    """fp64 at the fp64 bound"""
    f = chunk_problem()
    want, got = gradients(f, torch.float64, "shared", False, chain=False), gradients(f, torch.float64, "shared", True, chain=False)
    assert worst_ratio(got, want, lambda k, scale: 1e-12 * scale) <= 1.0


def test_two_backward_calls_give_the_same_bits():
    f = problem(70, "shared")
    a, b = gradients(f, torch.float32, "shared", True), gradients(f, torch.float32, "shared", True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
