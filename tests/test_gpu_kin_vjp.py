"""-m gpu: the fused backward of the inverse-kinematics implicit step (csrc/kin_vjp_kernels.hip: thx_kin_vjp; theseus_amd/kinematics.py:
PackedKinematics.assemble(graph=True)) against the torch path of the same packed class (``fused_backward = False``) evaluated in
fp64, with EVERY auxiliary tensor a leaf.  CPU twin: tests/test_kin_vjp_host.py.

fp64 bound: 1e-12 of each gradient's largest magnitude.  fp32: F32_FACTOR x the torch path's own fp32 distance from its fp64 value,
floored at F32_FLOOR of the largest magnitude."""
import functools

import numpy as np
import pytest
import torch

from tests.helpers import load_golden
from tests.kin_common import EE_NAME, FIXTURES, PANDA_URDF, TREE_URDF, chain_problem, has, make_model, pose_angle
from tests.push2_common import F32_FACTOR, F32_FLOOR
from tests.test_gpu_traj2_vjp import worst_ratio
from tests.test_kin_host import _lm, check_implicit_gradients

pytestmark = pytest.mark.gpu
DEV = "cuda"
AUX = ("pose_target", "w_pose", "pos_target", "w_pos", "hinge_down", "hinge_up", "hinge_thr", "w_hinge", "prior_target", "w_prior")
# (types, parents, pose link, position link, urdf, how far the pose target's angles lie from the start).  one_revolute: path length
# 1, and no position cost -- the link's origin lies on the only axis, so that cost's block is zero and the torch path's gradients of
# it are roundings of zero; tree: the links sit on different branches (paths of 4 joints, dof 6), so off-path columns exist
CHAINS = {
    "one_revolute": (["revolute"], [0], "link1", None, None, (0.3, 0.9)),
    "mix_fixed_end": (["revolute", "prismatic", "revolute", "fixed"], [0, 1, 2, 3], "link4", "link3", None, (0.3, 0.9)),
    "tree": (None, None, "tool_a", "tool_b", TREE_URDF, (0.2, 0.5)),
    "panda": (None, None, EE_NAME, "panda_link5", PANDA_URDF, (0.15, 0.4)),
}
# seeds for which ``assert_well_defined`` holds: (chain, B, targets shared) -> seed, 1 for every other case
SEEDS = {("one_revolute", 70, True): 2, ("mix_fixed_end", 70, True): 2, ("mix_fixed_end", 70, False): 2, ("tree", 70, True): 2,
         ("panda", 70, True): 6}
WIDTHS = {"w_pose": 6, "w_pos": 3, "w_hinge": None, "w_prior": None}   # (None: dof)


def objective(th, f, dtype, layout, device=DEV):
    """-> (objective, {name: the leaf that requires grad}): every auxiliary tensor is a leaf"""
    def t(key):
        return torch.from_numpy(np.asarray(f[key], np.float64)).to(dtype).to(device)
    links = [str(f[k]) for k in ("pose_link", "pos_link") if has(f, k)]
    model = make_model(th, f, dtype, device, links)
    leaves, aux = {}, {}
    for k in AUX:
        if not has(f, k):
            continue
        if layout == "sliced":   # the auxiliary is big[:, 1]: dense per problem, read through the parent's batch stride
            leaves[k] = torch.stack([t(k) - 7, t(k), t(k) + 7], dim=1).requires_grad_(True)
            aux[k] = leaves[k][:, 1]
        else:
            leaves[k] = aux[k] = t(k).requires_grad_(True)

    def weight(k):
        return (th.ScaleCostWeight if f[k].shape[-1] == 1 else th.DiagonalCostWeight)(th.Variable(aux[k], name=k))
    theta = th.Vector(tensor=t("theta_0"), name="theta")
    obj = th.Objective(dtype=dtype)
    obj.add(th.eb.LinkPoseCost(theta, th.SE3(tensor=aux["pose_target"], name="pose_target"), weight("w_pose"), model, links[0], name="pose"))
    if has(f, "pos_link"):
        obj.add(th.eb.LinkPositionCost(theta, th.Point3(tensor=aux["pos_target"], name="pos_target"), weight("w_pos"), model, links[1],
                                       name="pos"))
    obj.add(th.eb.HingeCost(theta, *[th.Variable(aux[k], name=k) for k in ("hinge_down", "hinge_up", "hinge_thr")], weight("w_hinge"),
                            name="limits"))
    obj.add(th.Difference(theta, th.Vector(tensor=aux["prior_target"], name="prior_target"), weight("w_prior"), name="prior"))
    return obj, leaves


def assert_well_defined(th, f, exact=0):
    """with the torch classes on the CPU in fp64: no kink of the reference within reach of an fp32 rounding (the first ``exact``
    problems have a zero pose error on purpose), and every hinge region occurs"""
    from theseus_amd.kernels import lie_eps
    switches = [x for d in (torch.float32, torch.float64) for x in (lie_eps(d).near_zero, lie_eps(d).d_near_zero)]
    obj, _ = objective(th, f, torch.float64, "batched", "cpu")
    a = pose_angle(obj.cost_functions["pose"])[exact:]
    assert 0.1 < float(a.min()) and float(a.max()) < np.pi - 0.1, (float(a.min()), float(a.max()))
    assert float(torch.stack([(a - x).abs() for x in switches]).min()) > 1e-5
    theta, down, up = f["theta_0"], f["hinge_down"] + f["hinge_thr"], f["hinge_up"] - f["hinge_thr"]
    assert min(np.abs(theta - down).min(), np.abs(theta - up).min()) >= 1e-3
    assert (theta < down).any() and ((theta > down) & (theta < up)).any() and np.isinf(f["hinge_up"]).any()
    assert (theta > up).any() or theta.shape[1] == 1   # (joint 0's upper limit is +inf: a robot with one joint is never above)


@functools.lru_cache(maxsize=None)
def problem(chain, B, layout, weights, exact=0):
    """chain_problem with all ten auxiliary tensors shared (1, ...) or per problem, Scale or Diagonal weights throughout, and a
    cotangent u; ``exact``: the pose targets of the first problems are fk(theta_0) itself"""
    import theseus_amd as th
    types, parents, pose_link, pos_link, urdf, away = CHAINS[chain]
    shared = layout == "shared"
    seed = SEEDS.get((chain, B, shared), 1)
    f = chain_problem(th, types, parents, pose_link, pos_link, B, seed, shared_targets=shared, urdf=urdf, away=away)
    dof = f["theta_0"].shape[1]
    for k, width in WIDTHS.items():
        if has(f, k):
            f[k] =np.linspace(0.6, 1.9, 1 if weights == "Scale" else (width or dof)).reshape(1, -1) + 0.1 * len(k)
    for k in AUX:
        if has(f, k) and not shared:
            f[k] = np.broadcast_to(f[k], (B,) + f[k].shape[1:]).copy()
    if exact:
        robot = make_model(th, f, torch.float64, "cpu", [pose_link]).robot
        with torch.no_grad():
            f["pose_target"][:exact] = robot.link_fk(torch.from_numpy(f["theta_0"][:exact]), pose_link, jacobian=False)[0].numpy()
    f["u"] = np.random.default_rng(seed).normal(0, 1, (B, dof))
    assert_well_defined(th, f, exact)
    return f


def gradients(f, dtype, layout, fused):
    """{leaf: d (g * u).sum() / d leaf as fp64 numpy} of ``packed.assemble(H, g, graph=True)``; fp32 inputs are f rounded to fp32"""
    import theseus_amd as th
    f = {k: a.astype(np.float32).astype(np.float64) if k in AUX + ("theta_0", "u") else a for k, a in f.items()}
    obj, leaves = objective(th, f, dtype, layout)
    lin = th.HipLinearization(obj)
    assert type(lin.packed).__name__ == "PackedKinematics" and type(lin.K).__name__ == "HipKernels"
    lin.packed.fused_backward = fused
    lin._ensure_buffers()
    g = lin.packed.assemble(lin._H, lin.g, graph=True)
    assert (type(g.grad_fn).__name__ == "_FusedGradientBackward") == fused
    (g * torch.from_numpy(f["u"]).to(dtype).to(DEV)).sum().backward()
    return {k: v.grad.double().cpu().numpy() for k, v in leaves.items()}


reference = functools.lru_cache(maxsize=None)(lambda dtype, *case: gradients(problem(*case), dtype, case[2], False))
F64_BOUND = lambda k, scale: 1e-12 * scale  # noqa: E731


@pytest.mark.parametrize("weights", ["Scale", "Diagonal"])
@pytest.mark.parametrize("layout", ["shared", "batched", "sliced"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("B", [3, 70])
@pytest.mark.parametrize("chain", list(CHAINS))
def test_gradients_of_every_auxiliary_tensor_match_the_torch_path(chain, B, dtype, layout, weights):
    """B = 3 is a partial wave; at B = 70 the second wave holds the end of one kind and the start of the next"""
    case = (chain, B, layout, weights)
    want = reference(torch.float64, *case)
    got = gradients(problem(*case), dtype, layout, True)
    assert set(got) == set(AUX) - ({"pos_target", "w_pos"} if chain == "one_revolute" else set())
    if chain == "one_revolute":   # its only upper limit is +inf: exactly 0 on both sides
        assert not want["hinge_up"].any() and not got["hinge_up"].any()
        want = {k: v for k, v in want.items() if k != "hinge_up"}
    if dtype == torch.float64:
        bound = F64_BOUND
    else:
        twin = reference(torch.float32, *case)
        bound = lambda k, scale: max(F32_FACTOR * float(np.abs(twin[k] - want[k]).max()), F32_FLOOR * scale)  # noqa: E731
    worst = worst_ratio(got, want, bound)
    print(f"kin_vjp {chain} {dtype} B={B} {layout} {weights}: worst difference / bound = {worst:.3f}")
    assert worst <= 1.0


def test_zero_residual_rotation_takes_the_small_angle_branch():
    """problem 0's pose target is fk(theta_0) exactly: log / Jlog take their Taylor branches and both sides define d sqrt at 0 as 0
    (se3_torch._safe_sqrt, csrc/dual.cuh); fp64 at the fp64 bound"""
    case = ("panda", 3, "batched", "Diagonal", 1)
    want, got = reference(torch.float64, *case), gradients(problem(*case), torch.float64, "batched", True)
    worst = worst_ratio(got, want, F64_BOUND)
    print(f"kin_vjp zero residual rotation: worst difference / bound = {worst:.3f}")
    assert worst <= 1.0


def test_two_backward_calls_give_the_same_bits():
    f = problem("panda", 70, "shared", "Diagonal")
    a, b = gradients(f, torch.float32, "shared", True), gradients(f, torch.float32, "shared", True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("fixture", FIXTURES)
def test_the_torch_classes_are_not_evaluated(fixture, monkeypatch):
    """implicit LM on the device with the fixture's leaves requiring grad: the reference's gradients, and no error() / jacobians()
    of a cost class (the pose target is fk of a leaf: autograd goes on through the forward kinematics)"""
    import theseus_amd as th

    def refuse(*a, **kw):
        raise AssertionError("a cost function was evaluated by torch although the family has a VJP kernel")
    for cls in (th.eb.LinkPoseCost, th.eb.LinkPositionCost, th.eb.HingeCost, th.Difference):
        for method in ("error", "jacobians"):
            monkeypatch.setattr(cls, method, refuse)
    g = load_golden(fixture)
    _, opt, leaves, sol, _ = _lm(th, g, None, device=DEV, backward_mode="implicit")
    assert type(opt.linear_solver.linearization.packed).__name__ == "PackedKinematics"
    check_implicit_gradients(g, leaves, sol)
