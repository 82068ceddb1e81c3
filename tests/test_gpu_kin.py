"""-m gpu: inverse kinematics on the fused kernels (csrc/kin_kernels.hip: thx_kin_eval, thx_kin_error; theseus_amd/kinematics.py:
PackedKinematics) against the torch classes and against the REAL reference's fixtures (tests/golden/kin_f64_*.npz).  CPU twin:
tests/test_kin_host.py.

Bounds of every comparison with the torch classes, per cost and per block (error vector / Jacobian block), against the FP64 class:
  fp64   REL[float64] = 1e-12 of the block's largest magnitude (tests/test_gpu_traj2.py)
  fp32   no fixed number: with dev = the largest deviation of the fp32 torch class from the fp64 torch class on the same input (the
         twin alone), the kernel may deviate max(4 * dev, 16 * eps32 * block max) -- 4 for another, equally valid operation order,
         the floor for blocks where the twin happens to be exact.  Both figures are printed.
The error metric 0.5 sum e^2 is bounded as in tests/test_gpu_homog.py, from the errors' own bounds a: sum |e| a + a^2 / 2, plus one
rounding of the result.  No test here reads the reference tree."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import load_golden
from tests.kin_common import EE_NAME, FIXTURES, GOLDEN, PANDA_URDF, TREE_URDF, build, chain_problem, pose_angle
from tests.test_gpu_traj2 import REL
from tests.test_kin_host import _lm, assert_blocks_close, check_implicit_gradients, check_iterates, run_implicit_with_nothing_to_differentiate
from theseus_amd.kinematics import KIN_TERM

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS32 = float(np.finfo(np.float32).eps)
both_dtypes = pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])


def _packed(th, obj):
    lin = th.HipLinearization(obj)
    assert type(lin.packed).__name__ == "PackedKinematics" and type(lin.K).__name__ == "HipKernels"
    return lin, lin.packed


def class_blocks(obj):
    """[(weighted block (B|1, dim, dof), weighted error (B|1, dim))] of the torch classes, in fp64 values"""
    out = []
    for cost in obj.cost_functions.values():
        jac, err = cost.weighted_jacobians_error()
        out.append((jac[0].double(), err.double()))
    return out


def compare(packed, want, twin=None):
    """thx_kin_eval's blocks and errors, thx_kin_error's metric <-> ``want`` = class_blocks of the fp64 objective; ``twin`` =
    class_blocks of the fp32 objective for an fp32 run"""
    Jv, ev = packed._eval()
    Jv, ev = [J[0].clone().double() for J in Jv], [e.clone().double() for e in ev]
    metric = packed.error_metric().double()
    B = packed.batch
    total = torch.zeros(B, dtype=torch.float64, device=DEV)
    slack = torch.zeros(B, dtype=torch.float64, device=DEV)
    worst = 0.0
    for c, cost in enumerate(packed.costs):
        for k, (got, what) in enumerate(((Jv[c], "block"), (ev[c], "error"))):
            ref = want[c][k].expand_as(got)
            top = float(ref.abs().max())
            diff = float((got - ref).abs().max())
            if twin is None:
                allowed = REL[torch.float64] * top
                print(f"{cost.name} {what}: {diff:.3e} (allowed {allowed:.3e} = 1e-12 of {top:.3e})")
            else:
                dev = float((twin[c][k].expand_as(got) - ref).abs().max())
                allowed = max(4 * dev, 16 * EPS32 * top)
                print(f"{cost.name} {what}: kernel {diff:.3e}, fp32 torch class {dev:.3e}, allowed {allowed:.3e}, "
                      f"ratio kernel / class {diff / dev if dev else float('inf'):.3f}")
            worst = max(worst, diff / allowed if allowed else 0.0)
            assert diff <= allowed, f"{cost.name} {what}: {diff:.3e} > {allowed:.3e}"
            if what == "error":
                total += (ref ** 2).sum(1)
                slack += ref.abs().sum(1) * allowed + 0.5 * ref.shape[1] * allowed ** 2
    ref = 0.5 * total
    slack = slack + (EPS32 if twin is not None else float(np.finfo(np.float64).eps)) * ref
    over = float(((metric - ref).abs() / slack).max())
    print(f"error metric: {over:.3e} of its bound; worst block {worst:.3e} of its bound")
    assert over <= 1.0
    return Jv, ev


def run_case(f, dtype, angles=(0.05, 3.0)):
    """build ``f`` in fp64 (the reference values) and in ``dtype`` -> (objective, packed, kernel blocks, kernel errors)"""
    import theseus_amd as th
    obj64, _, _, _ = build(th, f, device=DEV)
    if "pose" in obj64.cost_functions:
        a = pose_angle(obj64.cost_functions["pose"])
        assert angles[0] <= float(a.min()) and float(a.max()) <= angles[1], (float(a.min()), float(a.max()))
    with torch.no_grad():
        want = class_blocks(obj64)
        if dtype == torch.float64:
            obj, twin = obj64, None
        else:
            obj, _, _, _ = build(th, f, device=DEV, dtype=dtype)
            twin = class_blocks(obj)
        _, packed = _packed(th, obj)
        Jv, ev = compare(packed, want, twin)
    return obj, packed, Jv, ev


@both_dtypes
@pytest.mark.parametrize("fixture", FIXTURES)
def test_kernels_match_the_torch_classes_at_the_fixture_inputs(fixture, dtype):
    run_case(load_golden(fixture), dtype)


# dof 1 (with a fixed offset behind the joint, so that the link's position moves); dof 2 with a prismatic joint; a 9-joint path with fixed joints in the middle and at the end (7 dof) next to a short branch
CHAINS = {
    "dof1": (["revolute", "fixed"], [0, 1], "link2", "link2"),
    "dof2_prismatic": (["prismatic", "revolute"], [0, 1], "link2", "link1"),
    "path9_fixed_mid_and_end": (["revolute", "fixed", "prismatic", "revolute", "fixed", "continuous", "revolute", "revolute", "fixed",
                                 "revolute"], [0, 1, 2, 3, 4, 5, 6, 7, 8, 3], "link9", "link10"),
}


@both_dtypes
@pytest.mark.parametrize("B", [1, 3, 70, 300])
@pytest.mark.parametrize("chain", list(CHAINS))
def test_kernels_match_the_torch_classes_on_random_chains(chain, B, dtype):
    """B = 70 is past one wave, 300 past one 256-thread workgroup with the last one partial"""
    import theseus_amd as th
    types, parents, pose_link, pos_link = CHAINS[chain]
    away = (0.3, 0.9) if len(types) < 3 else (0.15, 0.4)
    _, packed, Jv, _ = run_case(chain_problem(th, types, parents, pose_link, pos_link, B, seed=3 + B, away=away), dtype)
    if chain == "path9_fixed_mid_and_end":
        robot = packed.robot
        assert robot.dof == 7 and len(robot.path("link9")) == 7 and robot.path("link9")[-1].kind == "fixed"
        # the branch link10 hangs on link3: the joints behind it on the long path are no ancestors -> exact zeros
        on = robot.link_map["link10"].ancestor_non_fixed_joint_ids
        off = [k for k in range(7) if k not in on]
        assert off and float(Jv[1][:, :, off].abs().sum()) == 0.0 and float(Jv[1][:, :, on].abs().min(0).values.max()) > 0
        off9 = [k for k in range(7) if k not in robot.link_map["link9"].ancestor_non_fixed_joint_ids]
        assert off9 and float(Jv[0][:, :, off9].abs().sum()) == 0.0


@both_dtypes
@pytest.mark.parametrize("B", [1, 3, 70, 300])
def test_kernels_match_the_torch_classes_on_the_panda(B, dtype):
    import theseus_amd as th
    run_case(chain_problem(th, None, None, EE_NAME, "panda_link5", B, seed=20 + B, urdf=PANDA_URDF, away=(0.15, 0.4)), dtype)


@both_dtypes
def test_two_link_terms_on_two_branches_share_their_ancestors(dtype):
    """tests/golden/kin_tree.urdf: tool_a behind joints 0, 1, 2, 4, tool_b behind 0, 1, 3, 5 -- the other columns are written as zeros"""
    import theseus_amd as th
    _, packed, Jv, _ = run_case(chain_problem(th, None, None, "tool_a", "tool_b", 70, seed=9, urdf=TREE_URDF, away=(0.2, 0.5)), dtype)
    assert packed.robot.link_map["tool_a"].ancestor_non_fixed_joint_ids == [0, 1, 2, 4]
    assert packed.robot.link_map["tool_b"].ancestor_non_fixed_joint_ids == [0, 1, 3, 5]
    assert float(Jv[0][:, :, [3, 5]].abs().sum()) == 0.0 == float(Jv[1][:, :, [2, 4]].abs().sum())
    # (joint 5 turns tool_b about its own origin: its position column is zero as well)
    assert float(Jv[0][:, :, [0, 1, 2, 4]].abs().amax((0, 1)).min()) > 0 and float(Jv[1][:, :, [0, 1, 3]].abs().amax((0, 1)).min()) > 0
    assert len(packed.path_of) == 2 and packed.path_of["tool_a"][0] == 0 and packed.path_of["tool_b"][0] == packed.path_of["tool_a"][1]


def test_zero_error_takes_the_small_angle_branch():
    """theta equals the target's configuration: the error is zero up to the rounding of two forward-kinematics chains, log and Jlog
    take their Taylor branches; fp64 only, absolute bound 1e-12"""
    import theseus_amd as th
    f = chain_problem(th, None, None, EE_NAME, None, 3, seed=31, urdf=PANDA_URDF, hinge=False, prior=False)
    robot = th.eb.Robot.from_urdf_file(os.path.join(GOLDEN, PANDA_URDF), dtype=torch.float64)
    with torch.no_grad():
        f["pose_target"] = robot.link_fk(torch.from_numpy(f["theta_0"]), EE_NAME, jacobian=False)[0].numpy()
        obj, _, _, _ = build(th, f, device=DEV)
        want = class_blocks(obj)
        _, packed = _packed(th, obj)
        Jv, ev = packed._eval()
        assert float(want[0][1].abs().max()) <= 1e-12 and float(ev[0].abs().max()) <= 1e-12
        diff = float((Jv[0][0] - want[0][0]).abs().max())
        print(f"zero-error block: {diff:.3e} (allowed 1e-12), error metric {float(packed.error_metric().max()):.3e}")
        assert diff <= 1e-12 and float(Jv[0][0].abs().max()) > 0.1
        assert float(packed.error_metric().max()) <= 1e-24


def _slice_targets(obj, dtype):
    """pose_target / pos_target / prior_target become slices ``big[:, 1]`` of (B, 2, ...) tensors whose other half holds values no
    cost should ever see"""
    for name in ("pose_target", "pos_target", "prior_target"):
        v = obj.get_variable(name)
        big = torch.full((v.shape[0], 2) + tuple(v.shape[1:]), -7.0, dtype=dtype, device=DEV)
        big[:, 1] = v.tensor
        v.tensor = big[:, 1]
        assert v.tensor[0].is_contiguous() and not v.tensor.is_contiguous()


@both_dtypes
def test_kernels_read_shared_and_sliced_auxiliaries_through_their_batch_stride(dtype):
    import theseus_amd as th
    f = chain_problem(th, None, None, "tool_a", "tool_b", 3, seed=6, urdf=TREE_URDF, shared_targets=True, away=(0.2, 0.5))
    _, packed, _, _ = run_case(f, dtype)   # targets of batch 1: stride 0
    table = packed._table.cpu().numpy().view(KIN_TERM)
    assert [int(t["kind"]) for t in table] == [0, 1, 2, 3] and all(int(t["aux_bstride"][0]) == 0 for t in table)
    f = chain_problem(th, None, None, "tool_a", "tool_b", 3, seed=6, urdf=TREE_URDF, away=(0.2, 0.5))
    obj64, _, _, _ = build(th, f, device=DEV)
    obj, _, _, _ = build(th, f, device=DEV, dtype=dtype)
    _slice_targets(obj, dtype)
    with torch.no_grad():
        _, packed = _packed(th, obj)
        compare(packed, class_blocks(obj64), None if dtype == torch.float64 else class_blocks(obj))
    table = packed._table.cpu().numpy().view(KIN_TERM)
    assert [int(table[k]["aux_bstride"][0]) for k in (0, 1, 3)] == [24, 6, 12] and packed._aux_key is not None


@both_dtypes
def test_two_calls_give_the_same_bits(dtype):
    import theseus_amd as th
    obj, _, _, _ = build(th, load_golden(FIXTURES[1]), device=DEV, dtype=dtype)
    _, packed = _packed(th, obj)
    runs = []
    for _ in range(2):
        packed._eval()
        runs.append((packed._J.clone(), packed._e.clone(), packed.error_metric().clone()))
        packed._J.fill_(7.0)
        packed._e.fill_(7.0)
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert bool(torch.isfinite(runs[0][0]).all()) and float(runs[0][0].abs().max()) > 0


@pytest.mark.parametrize("fixture", FIXTURES)
def test_fused_assemble_matches_the_reference(fixture):
    import theseus_amd as th
    g = load_golden(fixture)
    obj, _, _, _ = build(th, g, device=DEV)
    lin, packed = _packed(th, obj)
    lin.linearize()
    for c, name in enumerate(obj.cost_functions):
        assert_blocks_close(packed._Jv[c][0].cpu().numpy(), g[f"wj_{name}_0"], 1e-12, f"{name} block")
        assert_blocks_close(packed._ev[c].cpu().numpy(), g[f"we_{name}"], 1e-12, f"{name} error")
    assert_blocks_close(torch.tril(lin.AtA).cpu().numpy(), np.tril(g["AtA"]), 1e-12, "AtA")
    assert_blocks_close(lin.Atb.squeeze(2).cpu().numpy(), g["Atb"], 1e-12, "Atb")
    assert_blocks_close(obj.error_metric().cpu().numpy(), g["error_metric"], 1e-12, "error metric")


@pytest.mark.parametrize("fixture", FIXTURES)
def test_fused_lm_reproduces_the_reference_iterates(fixture):
    import theseus_amd as th
    g = load_golden(fixture)
    with torch.no_grad():
        _, opt, _, _, info = _lm(th, g, None, device=DEV, track_err_history=True, track_state_history=True)
    assert type(opt.linear_solver.linearization.packed).__name__ == "PackedKinematics"
    check_iterates(g, info, g["var_order"].tolist())


@pytest.mark.parametrize("fixture", FIXTURES)
def test_implicit_gradients_reproduce_the_reference(fixture):
    """w.r.t. the target angles, the position target and the prior target, through the torch twins"""
    import theseus_amd as th
    g = load_golden(fixture)
    _, opt, leaves, sol, _ = _lm(th, g, None, device=DEV, backward_mode="implicit")
    assert type(opt.linear_solver.linearization.packed).__name__ == "PackedKinematics"
    check_implicit_gradients(g, leaves, sol)


def test_implicit_mode_under_no_grad_stays_fused(monkeypatch):
    """the implicit last step with nothing to differentiate: thx_kin_eval + the gradient thx_block_assemble formed, no torch class"""
    import theseus_amd as th
    g = load_golden(FIXTURES[1])
    _, final = run_implicit_with_nothing_to_differentiate(th, g, None, monkeypatch, device=DEV)
    np.testing.assert_allclose(final.cpu().numpy(), g["implicit_final"], rtol=1e-8, atol=1e-10)


def test_the_fused_path_is_really_taken(monkeypatch):
    """No cost function is evaluated by torch in a no_grad LM run: one thx_kin_eval per linearization, thx_kin_error for every error
    metric."""
    import theseus_amd as th
    g = load_golden(FIXTURES[1])
    K = th.HipKernels()
    calls = {"kin_eval": 0, "kin_error": 0, "block_assemble_strided": 0}
    for name in calls:
        def counted(*a, _f=getattr(K, name), _n=name, **kw):
            calls[_n] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(K, name, counted)
    obj, _, _, _ = build(th, g, device=DEV)   # (the pose target is fk of the target angles: built before the classes are patched)

    def refuse(*a, **kw):
        raise AssertionError("a cost function was evaluated by torch on the fused path")
    for cls in (th.eb.LinkPoseCost, th.eb.LinkPositionCost, th.eb.HingeCost, th.Difference):
        for method in ("error", "jacobians"):
            monkeypatch.setattr(cls, method, refuse)
    linearizations = {"n": 0}
    real = th.HipLinearization._assemble

    def counting_assemble(self):
        linearizations["n"] += 1
        return real(self)
    monkeypatch.setattr(th.HipLinearization, "_assemble", counting_assemble)
    from tests.kin_common import LM_DAMPING, LM_KW
    opt = th.LevenbergMarquardt(obj, linearization_kwargs=dict(kernels=K), **LM_KW)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        with torch.no_grad():
            _, info = th.TheseusLayer(opt).forward(None, optimizer_kwargs=dict(damping=LM_DAMPING, track_err_history=True,
                                                                               track_state_history=True))
    finally:
        torch.set_default_dtype(old)
    assert opt.linear_solver.linearization.K is K
    assert linearizations["n"] >= 5 and calls["kin_eval"] == linearizations["n"] == calls["block_assemble_strided"]
    assert calls["kin_error"] >= 6   # the initial error + one per iteration
    check_iterates(g, info, g["var_order"].tolist())


def test_a_replaced_target_is_seen_by_the_next_call():
    """a new target tensor -> the table is rebuilt; values changed in place -> it is not"""
    import theseus_amd as th
    g = load_golden(FIXTURES[1])
    obj, _, _, _ = build(th, g, device=DEV)
    lin, packed = _packed(th, obj)
    lin.linearize()
    H0, e0 = lin.AtA.clone(), obj.error_metric().clone()
    with torch.no_grad():
        new_pose = obj.get_variable("pose_target").tensor.clone()
        new_pose[:, :, 3] += 0.05
        new_pos = torch.from_numpy(g["pos_target"]).to(DEV) + 0.1
    obj.update({"pose_target": new_pose, "pos_target": new_pos})
    lin.linearize()
    assert float((lin.AtA - H0).abs().max()) > 1e-4 and float((obj.error_metric() - e0).abs().max()) > 1e-4
    with torch.no_grad():
        compare(packed, class_blocks(obj))
        table = packed._table
        new_pose[:, :, 3] -= 0.02
        new_pos.add_(0.02)
        compare(packed, class_blocks(obj))
    assert packed._table is table
