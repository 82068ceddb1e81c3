"""-m gpu: the fused backward of the homography family's implicit step (csrc/homog_vjp_kernels.hip: thx_homog_vjp;
theseus_amd/homography.py) against the torch route of the same packed class (``fused_backward = False``) evaluated in fp64.
CPU twin: tests/test_homog_vjp_host.py."""
import functools

import numpy as np
import pytest
import torch

from tests.helpers import load_golden
from tests.homog_common import MARGIN, kernel_problem, min_margin
from tests.test_gpu_traj2_vjp import worst_ratio
from tests.test_homog_host import _lm, check_implicit_gradients

pytestmark = pytest.mark.gpu
DEV = "cuda"
LEAVES = ("feat_src", "feat_dst", "w_align", "H8_prior", "w_prior")
# a map far smaller than a chunk; two sort chunks and a 32-pixel tail, C next to the channel slice of 4; a partial second slice
SHAPES = [(1, 5, 9), (3, 33, 32), (5, 6, 7)]


@functools.lru_cache(maxsize=None)
def gradients(B, shape, dtype, layout, fused, scale=1.0):
    """{leaf: d (g * u).sum() / d leaf as fp64 numpy} of ``packed.assemble(H, g, graph=True)`` on kernel_problem(B, *shape); fp32
    inputs are the fp64 ones rounded to fp32.  Never modified by the tests."""
    import theseus_amd as th
    C, Hh, Ww = shape
    f = kernel_problem(B, C, Hh, Ww, seed=7 + Hh, scale=scale)

    def t(key):
        return torch.from_numpy(f[key].astype(np.float32).astype(np.float64)).to(dtype).to(DEV)
    leaves, aux = {}, {}
    for k in LEAVES:
        if layout == "sliced" and t(k).shape[0] == B:   # the auxiliary is big[:, 1]: dense per problem, read through the batch stride
            leaves[k] = torch.stack([t(k) - 7, t(k), t(k) + 7], dim=1).requires_grad_(True)
            aux[k] = leaves[k][:, 1]
        else:
            leaves[k] = aux[k] = t(k).requires_grad_(True)
    H8 = th.Vector(tensor=t("H8_0"), name="H8")
    obj = th.Objective(dtype=dtype)
    obj.add(th.eb.HomographyAlignment(H8, th.Variable(aux["feat_src"], name="feat_src"), th.Variable(aux["feat_dst"], name="feat_dst"),
                                      th.ScaleCostWeight(th.Variable(aux["w_align"], name="w_align")), name="align"))
    obj.add(th.Difference(H8, th.Vector(tensor=aux["H8_prior"], name="H8_prior"),
                          th.DiagonalCostWeight(th.Variable(aux["w_prior"], name="w_prior")), name="prior"))
    if dtype == torch.float32:
        assert min_margin(obj.cost_functions["align"]) >= MARGIN
    lin = th.HipLinearization(obj)
    assert type(lin.packed).__name__ == "PackedHomography" and type(lin.K).__name__ == "HipKernels"
    lin.packed.fused_backward = fused
    lin._ensure_buffers()
    g = lin.packed.assemble(lin._H, lin.g, graph=True)
    assert (type(g.grad_fn).__name__ == "_FusedGradientBackward") == fused   # (the route under test was the one taken)
    u = np.random.default_rng(3).normal(0, 1, (B, 8))
    (g * torch.from_numpy(u).to(dtype).to(DEV)).sum().backward()
    assert H8.tensor.grad is None
    return {k: v.grad.double().cpu().numpy() for k, v in leaves.items()}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("layout", ["batched", "sliced"])
@pytest.mark.parametrize("B", [1, 3, 70])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_gradients_of_every_auxiliary_tensor_match_the_torch_route(dtype, B, layout, shape):
    """fp64: 1e-12 of each gradient's largest magnitude.  fp32: 4 x the torch route's own fp32 distance from its fp64 value, floored
    at 16 * 2^-23 of the largest magnitude (the pushing family's rule)."""
    want = gradients(B, shape, torch.float64, layout, False)
    got = gradients(B, shape, dtype, layout, True)
    if dtype == torch.float64:
        bound = lambda k, scale: 1e-12 * scale  # noqa: E731
    else:
        twin = gradients(B, shape, torch.float32, layout, False)
        bound = lambda k, scale: max(4 * float(np.abs(twin[k] - want[k]).max()), 16 * 2.0 ** -23 * scale)  # noqa: E731
    worst = worst_ratio(got, want, bound)
    print(f"homog_vjp {dtype} B={B} {layout} {shape}: worst difference / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("scale", [3.0, 0.25])
def test_warps_that_collapse_many_pixels_onto_one_cell(scale):
    """scale 3: a third of the pixels leave the image on each side and clamp onto border cells, through two or four coinciding
    corners; scale 0.25: sixteen destination pixels per source cell.  fp64 bound."""
    want = gradients(2, (2, 33, 32), torch.float64, "batched", False, scale)
    got = gradients(2, (2, 33, 32), torch.float64, "batched", True, scale)
    assert worst_ratio(got, want, lambda k, s: 1e-12 * s) <= 1.0


def _watch(th, monkeypatch, refuse):
    calls = {"n": 0}
    for cls in (th.eb.HomographyAlignment, th.Difference):
        def watched(self, _real=cls.weighted_jacobians_error):
            calls["n"] += 1
            assert not refuse, "a cost function was evaluated by torch although the family has a VJP kernel"
            return _real(self)
        monkeypatch.setattr(cls, "weighted_jacobians_error", watched)
    return calls


def test_the_torch_classes_are_not_evaluated(monkeypatch):
    """implicit LM on the device with the batched fixture's leaves requiring grad: the reference's gradients, and no
    weighted_jacobians_error"""
    import theseus_amd as th
    _watch(th, monkeypatch, refuse=True)
    g = load_golden("homog_f64_batched")
    _, opt, leaves, sol, _ = _lm(th, g, None, device=DEV, backward_mode="implicit")
    assert type(opt.linear_solver.linearization.packed).__name__ == "PackedHomography"
    check_implicit_gradients(g, leaves, sol)


def test_a_shared_feature_map_that_requires_grad_takes_the_torch_route(monkeypatch):
    import theseus_amd as th
    calls = _watch(th, monkeypatch, refuse=False)
    g = load_golden("homog_f64_shared")
    _, opt, leaves, sol, _ = _lm(th, g, None, device=DEV, backward_mode="implicit")
    assert type(opt.linear_solver.linearization.packed).__name__ == "PackedHomography" and calls["n"] >= 2
    check_implicit_gradients(g, leaves, sol)


def test_two_backward_calls_give_the_same_bits():
    a = gradients(70, (3, 33, 32), torch.float32, "batched", True)
    b = gradients.__wrapped__(70, (3, 33, 32), torch.float32, "batched", True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
