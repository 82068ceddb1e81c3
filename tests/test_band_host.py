"""CPU-side (-m "not gpu") checks of the banded Cholesky solver: the C entry points refuse bad arguments before any launch; header,
library, ctypes table and INTEGRATION.md agree on the three names; the band plan of the trajectory fixtures; the solver's host
logic on the numpy stand-in of the three kernels (tests/band_oracle_kernels.py); the plugin adapter is a th.CholeskyDenseSolver
for the reference's isinstance whitelists (where the reference imports)."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests.helpers import load_golden
from tests.test_cabi_and_host import declared_symbols, lib_path  # noqa: F401  (lib_path: the session fixture that builds)
from tests.test_traj2_host import check_implicit_gradients, check_iterates
from tests import traj2_common, trajse2_common
from tests.traj2_common import LM_DAMPING, LM_KW, build

BAND_NAMES = ["thx_band_factor", "thx_band_solve", "thx_band_solve_backward"]
REF = os.environ.get("THX_REFERENCE_ROOT", "/root/reference")
needs_reference = pytest.mark.skipif(not os.path.isdir(REF), reason="needs /root/reference")


def test_bad_arguments_to_the_band_entry_points_are_refused_before_any_launch(lib_path):  # noqa: F811
    from theseus_amd import _lib
    lib = _lib.load()
    one, two, three = ctypes.c_void_p(16), ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    lim = _lib.THX_BAND_MAX_KD
    assert lim == 63
    # thx_band_factor(H, ld, n, kd, B, perm, damping, ellipsoidal, eps, Lb, info, rhs, y, ldv, dtype, stream)
    f = lib.thx_band_factor
    for bad in ((None, one, two, three), (one, None, two, three), (one, one, None, three), (one, one, two, None)):
        H, perm, Lb, info = bad
        assert f(H, 32, 6, 2, 1, perm, None, 0, 1e-8, Lb, info, None, None, 6, 0, None) != 0 and b"null pointer" in lib.thx_last_error()
    assert f(one, 32, 6, 2, 1, one, None, 0, 1e-8, two, three, one, None, 6, 0, None) != 0 and b"null pointer" in lib.thx_last_error()
    assert f(one, 32, 6, 6, 1, one, None, 0, 1e-8, two, three, None, None, 6, 0, None) != 0 and b"kd" in lib.thx_last_error()   # kd >= n
    assert f(one, 32, 6, -1, 1, one, None, 0, 1e-8, two, three, None, None, 6, 0, None) != 0 and b"kd" in lib.thx_last_error()
    assert f(one, 128, 100, lim + 1, 1, one, None, 0, 1e-8, two, three, None, None, 100, 0, None) != 0
    assert b"limit" in lib.thx_last_error() and str(lim).encode() in lib.thx_last_error()
    assert f(one, 5, 6, 2, 1, one, None, 0, 1e-8, two, three, None, None, 6, 0, None) != 0 and b"ld < n" in lib.thx_last_error()
    assert f(one, 32, 6, 2, 1, one, None, 0, 1e-8, two, three, one, two, 5, 0, None) != 0 and b"ldv" in lib.thx_last_error()
    assert f(one, 32, 6, 2, 1, one, None, 0, 1e-8, two, three, None, None, 6, 7, None) != 0 and b"dtype" in lib.thx_last_error()
    assert f(one, 32, 6, 2, 1, one, None, 0, 1e-8, one, three, None, None, 6, 0, None) != 0 and b"alias" in lib.thx_last_error()
    # the solves: (Lb, n, kd, B, perm, rhs | y, x, ldv, dtype, stream)
    for s in (lib.thx_band_solve, lib.thx_band_solve_backward):
        for bad in ((None, one, two, three), (one, None, two, three), (one, one, None, three), (one, one, two, None)):
            Lb, perm, rhs, x = bad
            assert s(Lb, 6, 2, 1, perm, rhs, x, 6, 0, None) != 0 and b"null pointer" in lib.thx_last_error()
        assert s(one, 6, 6, 1, one, two, three, 6, 0, None) != 0 and b"kd" in lib.thx_last_error()
        assert s(one, 100, lim + 1, 1, one, two, three, 100, 0, None) != 0 and str(lim).encode() in lib.thx_last_error()
        assert s(one, 6, 2, 1, one, two, three, 5, 0, None) != 0 and b"ldv" in lib.thx_last_error()
        assert s(one, 6, 2, 1, one, two, three, 6, 7, None) != 0 and b"dtype" in lib.thx_last_error()


def test_header_library_ctypes_table_and_build_agree_on_the_band_names(lib_path):  # noqa: F811
    from theseus_amd import _lib, build as thx_build
    assert [s for s in declared_symbols() if s.startswith("thx_band_")] == BAND_NAMES
    assert [s for s in _lib.EXPORTED_SYMBOLS if s.startswith("thx_band_")] == BAND_NAMES
    lib = ctypes.CDLL(lib_path)
    assert all(hasattr(lib, s) for s in BAND_NAMES)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(s in doc for s in BAND_NAMES)
    assert _lib.ABI_VERSION == 30 and lib.thx_abi_version() == 30
    assert "band_kernels.hip" in thx_build.SOURCES
    header = open(os.path.join(ROOT, "include", "theseus_hip.h")).read()
    assert f"#define THX_BAND_MAX_KD {_lib.THX_BAND_MAX_KD}" in header


def test_banded_solver_is_exported_with_the_cholesky_solvers_constructor():
    import theseus_amd as th
    from theseus_amd.linear_solver import DenseCholeskyOnly, HipBandedCholeskyCore, HipCholeskyCore
    assert issubclass(th.HipBandedCholeskySolver, HipBandedCholeskyCore) and issubclass(HipBandedCholeskyCore, DenseCholeskyOnly)
    assert list(inspect.signature(th.HipBandedCholeskySolver.__init__).parameters) == \
        list(inspect.signature(th.HipCholeskySolver.__init__).parameters)
    # the surface the loops and the autograd nodes call on the Cholesky core (tests/test_lu_host.py lists it for the LU core)
    for name in ("factorize", "_substitute", "solve_with_factor", "factor_snapshot", "solve_with_snapshot", "check_info",
                 "singular_mask", "dropped_mask", "post_singular_warning", "_solve"):
        assert callable(getattr(HipBandedCholeskyCore, name)) and callable(getattr(HipCholeskyCore, name)), name
    assert HipBandedCholeskyCore.check_info is HipCholeskyCore.check_info   # one RuntimeError text for a failed item
    with pytest.raises(RuntimeError, match="HipBandedCholeskySolver only works with theseus_amd.HipLinearization"):
        th.HipBandedCholeskySolver(th.Objective(), linearization_cls=dict)
    with pytest.raises(ValueError, match="ordering"):
        th.HipBandedCholeskySolver(th.Objective(), ordering="amd")
    # no default changes: the optimizers still pick the dense solver
    obj, _, _ = build(th, load_golden(traj2_common.FIXTURES[0]))
    from tests.traj2_oracle_kernels import Traj2OracleKernels
    opt = th.LevenbergMarquardt(obj, linearization_kwargs=dict(kernels=Traj2OracleKernels()), **LM_KW)
    assert type(opt.linear_solver) is th.HipCholeskySolver


# ---- the band plan ------------------------------------------------------------------------------------------------------------
def _solver(th, common, fixture, K, **kw):
    obj, _, _ = common.build(th, load_golden(fixture))
    return th.HipBandedCholeskySolver(obj, linearization_kwargs=dict(kernels=K), **kw)


def _pattern_bandwidth(lin, perm):
    """half-bandwidth of the NUMERIC tril(AtA) under perm (independent of the plan's own arithmetic)"""
    lin.linearize()
    A = lin.AtA[:, perm][:, :, perm]
    r, c = np.nonzero((A != 0).any(dim=0).numpy())
    return int(np.abs(r - c).max())


@pytest.mark.parametrize("family,n,kd_rcm,kd_nat", [("traj2", 28, 7, 23), ("trajse2", 36, 11, 29)])
def test_band_plan_of_the_trajectory_fixtures(family, n, kd_rcm, kd_nat):
    import theseus_amd as th
    from tests.band_oracle_kernels import BandTraj2OracleKernels, BandTrajSE2OracleKernels
    common, K = {"traj2": (traj2_common, BandTraj2OracleKernels), "trajse2": (trajse2_common, BandTrajSE2OracleKernels)}[family]
    for fixture in common.FIXTURES:
        solver = _solver(th, common, fixture, K())
        assert type(solver.linearization.packed).__name__ == {"traj2": "PackedTrajectory2D", "trajse2": "PackedTrajectorySE2"}[family]
        plan = solver.band_plan()
        perm, kd, pn = plan
        assert pn == n == solver.linearization.n and kd <= kd_rcm and plan is solver.band_plan()
        assert perm.dtype == np.int32 and sorted(perm.tolist()) == list(range(n))
        assert _pattern_bandwidth(solver.linearization, perm.astype(np.int64)) <= kd
        natural = _solver(th, common, fixture, K(), ordering="natural").band_plan()
        assert natural.kd == kd_nat and natural.perm.tolist() == list(range(n))
        assert _pattern_bandwidth(solver.linearization, np.arange(n)) == kd_nat


def test_band_plan_keeps_a_natural_order_that_is_no_wider():
    """a chain added in order: reverse Cuthill-McKee cannot do better, the identity stays"""
    import theseus_amd as th
    from tests.band_oracle_kernels import BandOracleKernels
    obj = th.Objective(dtype=torch.float64)
    vs = [th.Vector(tensor=torch.zeros(2, 3, dtype=torch.float64), name=f"v{k}") for k in range(5)]
    w = th.ScaleCostWeight(torch.tensor(1.0, dtype=torch.float64))
    obj.add(th.Difference(vs[0], th.Vector(tensor=torch.ones(2, 3, dtype=torch.float64), name="t"), w, name="prior"))
    for k in range(4):
        obj.add(th.AutoDiffCostFunction([vs[k], vs[k + 1]], lambda optim_vars, aux_vars: optim_vars[1].tensor - optim_vars[0].tensor - 1.0,
                                        3, name=f"b{k}"))
    plan = th.HipBandedCholeskySolver(obj, linearization_kwargs=dict(kernels=BandOracleKernels())).band_plan()
    assert plan.kd == 5 and plan.n == 15 and plan.perm.tolist() == list(range(15))


def test_a_dense_pattern_above_the_limit_is_refused_with_kd_and_the_limit():
    import theseus_amd as th
    from theseus_amd import _lib
    from tests.band_oracle_kernels import BandOracleKernels
    obj = th.Objective(dtype=torch.float64)
    v = th.Vector(tensor=torch.zeros(2, 70, dtype=torch.float64), name="v")
    obj.add(th.AutoDiffCostFunction([v], lambda optim_vars, aux_vars: optim_vars[0].tensor.cumsum(1) - 1.0, 70, name="dense"))
    solver = th.HipBandedCholeskySolver(obj, linearization_kwargs=dict(kernels=BandOracleKernels()))
    with pytest.raises(th.UnsupportedObjective, match=rf"kd = 69 .*limit of {_lib.THX_BAND_MAX_KD}.*HipCholeskySolver"):
        solver.band_plan()
    solver.linearization.linearize()
    with pytest.raises(NotImplementedError, match="kd = 69"):   # (UnsupportedObjective is one) -- and from solve() as well
        solver.solve()


def test_a_system_handed_over_as_plain_tensors_is_refused():
    from theseus_amd.banded import band_plan

    class Lin:
        full_matrix = torch.eye(3).unsqueeze(0)
    with pytest.raises(NotImplementedError, match="plain tensors"):
        band_plan(Lin())


def test_band_plan_rejects_what_is_not_a_permutation():
    from theseus_amd.banded import BandPlan
    with pytest.raises(ValueError, match="permutation"):
        BandPlan(np.array([0, 2, 2]), 1, 3)


# ---- the solver on the stand-in kernels ---------------------------------------------------------------------------------------
def _lm(th, common, g, kernels, device="cpu", **okw):
    obj, leaves, _ = common.build(th, g, device=device, grad=bool(okw.get("backward_mode")))
    opt = th.LevenbergMarquardt(obj, linear_solver_cls=th.HipBandedCholeskySolver,
                                linearization_kwargs=dict(kernels=kernels) if kernels is not None else {}, **common.LM_KW)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)   # (info.state_history is kept in the default dtype, as the reference keeps it)
    try:
        sol, info = th.TheseusLayer(opt).forward(None, optimizer_kwargs=dict(damping=common.LM_DAMPING, **okw))
    finally:
        torch.set_default_dtype(old)
    return obj, opt, leaves, sol, info


@pytest.mark.parametrize("fixture", traj2_common.FIXTURES)
def test_banded_lm_on_the_stand_in_kernels_reproduces_the_reference(fixture):
    import theseus_amd as th
    from tests.band_oracle_kernels import BandTraj2OracleKernels
    assert LM_DAMPING == traj2_common.LM_DAMPING
    g = load_golden(fixture)
    with torch.no_grad():
        _, opt, _, _, info = _lm(th, traj2_common, g, BandTraj2OracleKernels(), track_err_history=True, track_state_history=True)
    assert type(opt.linear_solver) is th.HipBandedCholeskySolver and opt.linear_solver.band_plan().kd <= 7
    assert type(opt.linear_solver.linearization.packed).__name__ == "PackedTrajectory2D"
    assert tuple(opt.linear_solver.Lb.shape) == (3, 28, opt.linear_solver.band_plan().kd + 1)
    check_iterates(g, info, g["var_order"].tolist())
    _, _, leaves, sol, _ = _lm(th, traj2_common, g, BandTraj2OracleKernels(), backward_mode="implicit")
    check_implicit_gradients(g, leaves, sol, g["var_order"].tolist())


def test_banded_unrolled_gradients_equal_the_dense_solvers():
    import theseus_amd as th
    from tests.band_oracle_kernels import BandTraj2OracleKernels
    from tests.test_traj2_host import _lm as dense_lm
    from tests.traj2_common import state_of
    g = load_golden(traj2_common.FIXTURES[1])
    names = g["var_order"].tolist()
    _, _, leaves, sol, _ = _lm(th, traj2_common, g, BandTraj2OracleKernels(), backward_mode="unroll")
    (state_of(sol, names) ** 2).sum().backward()
    _, _, dleaves, dsol, _ = dense_lm(th, g, BandTraj2OracleKernels(), backward_mode="unroll")
    (state_of(dsol, names) ** 2).sum().backward()
    for k, leaf in dleaves.items():
        want = leaf.grad.numpy()
        assert np.abs(want).max() > 0
        np.testing.assert_allclose(leaves[k].grad.numpy(), want, rtol=0, atol=1e-9 * np.abs(want).max(), err_msg=k)


def test_the_multi_right_hand_side_surface_raises_and_a_failed_item_raises_the_cholesky_error():
    import theseus_amd as th
    from tests.band_oracle_kernels import BandTraj2OracleKernels
    solver = _solver(th, traj2_common, traj2_common.FIXTURES[0], BandTraj2OracleKernels())
    solver.linearization.linearize()
    with pytest.raises(NotImplementedError, match="HipCholeskySolver"):
        solver.sample_deltas(2)
    with pytest.raises(NotImplementedError):
        solver.marginal_covariance(["pose_1"])
    with pytest.raises(NotImplementedError):
        solver.solve_multi_with_factor(torch.zeros(3, 1, 28, dtype=torch.float64))
    delta = solver.solve(0.1)
    A = solver.linearization.AtA
    damped = A + torch.diag_embed(0.1 * A.diagonal(dim1=1, dim2=2) + 1e-8)
    np.testing.assert_allclose((damped @ delta.unsqueeze(2)).squeeze(2).numpy(), solver.linearization.g.numpy(), rtol=1e-9, atol=1e-9)
    w = solver.solve_with_factor(delta)
    np.testing.assert_allclose((damped @ w.unsqueeze(2)).squeeze(2).numpy(), delta.numpy(), rtol=1e-9, atol=1e-9)
    k = int(solver.band_plan().perm[3])
    solver.linearization.H[1, k, k] = -1.0
    with pytest.raises(RuntimeError, match=r"Batch element 1.*leading minor of order 4 is not positive-definite"):
        solver.solve()


# ---- the plugin adapter -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref():
    for p in (os.path.join(ROOT, "oracle", "stubs"), REF, REF + "/torchlie", REF + "/torchkin"):
        if p not in sys.path:
            sys.path.append(p)
    import warnings
    warnings.filterwarnings("ignore")
    import theseus as th
    import theseus_amd.plugin as thp
    return th, thp


@needs_reference
@pytest.mark.reference
def test_plugin_banded_solver_passes_the_reference_whitelists(ref):
    from tests.band_oracle_kernels import BandOracleKernels
    from tests.test_lu_host import _tiny_objective
    th, thp = ref
    obj = _tiny_objective(th)
    solver = thp.HipBandedCholeskySolver(obj, linearization_kwargs=dict(kernels=BandOracleKernels()))
    assert isinstance(solver, th.CholeskyDenseSolver) and not isinstance(solver, th.LUDenseSolver)
    opt = th.LevenbergMarquardt(obj, linear_solver_cls=thp.HipBandedCholeskySolver, linearization_kwargs=dict(kernels=BandOracleKernels()),
                                max_iterations=3, step_size=1.0)
    assert isinstance(opt.linear_solver, thp.HipBandedCholeskySolver)
    assert opt._allows_ellipsoidal and opt._allows_adaptive
    obj.update({})
    with torch.no_grad():
        opt.optimize(damping=0.01)
    np.testing.assert_allclose(obj.get_optim_var("a").tensor.numpy(), np.ones((2, 3)), atol=1e-4)
    assert opt.linear_solver.band_plan().kd == 2
    with pytest.raises(RuntimeError, match="HipBandedCholeskySolver only works with theseus_amd.plugin.HipLinearization"):
        thp.HipBandedCholeskySolver(_tiny_objective(th), linearization_cls=th.DenseLinearization)
