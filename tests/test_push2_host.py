"""CPU-side (-m "not gpu") checks of planar pushing on SE2 (theseus_amd/se2_torch.py, the three cost classes of
theseus_amd/embodied.py, theseus_amd/pushing.py, csrc/push_kernels.hip): the torch SE2 functions against the reference's Lie
fixture and under gradcheck, the torch classes and the packer (on a numpy stand-in of the two kernels) against the REAL reference's
fixtures (tests/golden/push2_f64_*.npz, tools/gen_push2_golden.py), the C ABI of the two new exports, their argument checks (through
ctypes and in a stand-alone program under the host sanitizers), and which packed family ``packed_for`` selects.  GPU twin:
tests/test_gpu_push2.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests.helpers import load_golden
from tests.push2_common import ALL_CASES, FIXTURES, LM_DAMPING, LM_KW, build, classify, state_of
from tests.test_cabi_and_host import declared_symbols, lib_path  # noqa: F401  (lib_path: the session fixture that builds)
from tests.test_traj2_host import assert_blocks_close

NAMES = ("thx_push2_eval", "thx_push2_error")


# ---- the torch SE2 functions ---------------------------------------------------------------------------------------------------
def test_se2_torch_functions_match_the_reference_lie_fixture():
    """tests/test_oracle_golden.py's tolerance for the SE2 operations in fp64"""
    from theseus_amd import se2_torch as S
    g = load_golden("lie_se2_f64")
    xi, X, Y = (torch.from_numpy(g[k]) for k in ("xi", "exp", "Y"))
    tol = dict(rtol=1e-12, atol=1e-12)
    e, je = S.exp(xi, jac=True)
    np.testing.assert_allclose(e.numpy(), g["exp"], **tol)
    np.testing.assert_allclose(je.numpy(), g["jexp"], **tol)
    lg, jl = S.log(X, jac=True)
    np.testing.assert_allclose(lg.numpy(), g["log"], **tol)
    np.testing.assert_allclose(jl.numpy(), g["jlog"], **tol)
    np.testing.assert_allclose(S.adjoint(X).numpy(), g["adj"], **tol)
    np.testing.assert_allclose(S.inverse(X).numpy(), g["inv"], **tol)
    np.testing.assert_allclose(S.compose(X, Y).numpy(), g["compose"], **tol)
    np.testing.assert_allclose(S.between(X, Y).numpy(), S.compose(torch.from_numpy(g["inv"]), Y).numpy(), **tol)
    np.testing.assert_allclose(S.theta(X).numpy()[:, 0], g["log"][:, 2], **tol)


def _poses(n, seed):
    gen = torch.Generator().manual_seed(seed)
    v = torch.randn(n, 3, dtype=torch.float64, generator=gen)
    return torch.cat([v[:, :2], v[:, 2:].cos(), v[:, 2:].sin()], dim=1)


def test_se2_torch_functions_pass_gradcheck():
    """Autograd goes through every function (values and Jacobians), away from the Taylor switches; the analytic Jacobians are the
    derivatives w.r.t. a right perturbation of the argument: checked against autograd through retract."""
    from theseus_amd import se2_torch as S
    A, B = _poses(4, 1).requires_grad_(), _poses(4, 2).requires_grad_()
    xi = torch.randn(4, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(3)).requires_grad_()
    p = torch.randn(4, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(4)).requires_grad_()
    gc = torch.autograd.gradcheck
    assert gc(lambda x: S.exp(x, jac=True), (xi,))
    assert gc(lambda a: S.log(a, jac=True), (A,))
    assert gc(lambda a: S.inverse(a, jac=True), (A,))
    assert gc(lambda a: S.adjoint(a), (A,))
    assert gc(lambda a, b: (lambda r: (r[0],) + r[1])(S.compose(a, b, jac=True)), (A, B))
    assert gc(lambda a, b: (lambda r: (r[0],) + r[1])(S.between(a, b, jac=True)), (A, B))
    assert gc(lambda a, b: (lambda r: (r[0],) + r[1])(S.local(a, b, jac=True)), (A, B))
    assert gc(lambda a: S.xy(a, jac=True), (A,))
    assert gc(lambda a: S.theta(a), (A,))
    assert gc(lambda a, q: (lambda r: (r[0],) + r[1])(S.transform_to(a, q, jac=True)), (A, p))
    assert gc(lambda a, q: (lambda r: (r[0],) + r[1])(S.unrotate(a[:, 2:], q, jac=True)), (A, p))
    assert gc(lambda a, d: S.retract(a, d), (A, xi))

    def right_jacobian(f, X, dim):   # d f(X exp(d)) / d d at d = 0, by autograd
        d0 = torch.zeros(X.shape[0], 3, dtype=torch.float64)
        J = torch.autograd.functional.jacobian(lambda d: f(S.retract(X, d)).sum(0), d0)   # (dim, B, 3)
        return J.permute(1, 0, 2)
    Ad, Bd = A.detach(), B.detach()
    close = lambda a, b: np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-9, atol=1e-9)  # noqa: E731
    close(S.log(Ad, jac=True)[1], right_jacobian(S.log, Ad, 3))
    close(S.xy(Ad, jac=True)[1], right_jacobian(S.xy, Ad, 2))
    close(S.theta(Ad, jac=True)[1], right_jacobian(S.theta, Ad, 1))
    close(S.transform_to(Ad, p.detach(), jac=True)[1][0], right_jacobian(lambda x: S.transform_to(x, p.detach()), Ad, 2))
    close(S.local(Ad, Bd, jac=True)[1][0], right_jacobian(lambda x: S.local(x, Bd), Ad, 3))
    close(S.local(Ad, Bd, jac=True)[1][1], right_jacobian(lambda x: S.local(Ad, x), Bd, 3))
    # between / compose / inverse map to the group: their Jacobians relate right perturbations, log(f(X)^-1 f(X exp(d)))
    for f, X, want in ((lambda x: S.between(x, Bd), Ad, S.between(Ad, Bd, jac=True)[1][0]),
                       (lambda x: S.compose(x, Bd), Ad, S.compose(Ad, Bd, jac=True)[1][0]),
                       (lambda x: S.inverse(x), Ad, S.inverse(Ad, jac=True)[1])):
        base = f(X)
        close(want, right_jacobian(lambda x: S.log(S.between(base, f(x))), X, 3))


def test_se2_torch_taylor_switches_follow_the_kernels_thresholds():
    import theseus_amd as th
    from theseus_amd import se2_torch as S
    xi = torch.tensor([[0.3, -0.2, 5e-4]], dtype=torch.float64)
    near = S.exp(xi)
    th.set_se2_eps(torch.float64, near_zero=1e-3)
    try:
        taylor = S.exp(xi)
    finally:
        th.reset_global_params()
    assert not torch.equal(near, taylor) and float((near - taylor).abs().max()) < 1e-9
    assert torch.equal(S.exp(xi), near)


# ---- the cost classes and the packer against the reference's fixtures -------------------------------------------------------------
@pytest.mark.parametrize("fixture", FIXTURES)
def test_torch_classes_reproduce_the_reference_blocks(fixture):
    """Each value is a few hundred flops on inputs of order 1: 1e-12 of the block's largest magnitude (the bound of
    tests/test_traj2_host.py) is far above fp64 rounding and far below any formula error."""
    import theseus_amd as th
    g = load_golden(fixture)
    obj, _, costs = build(th, g)
    assert costs == g["cost_order"].tolist() and list(obj.optim_vars) == g["var_order"].tolist()
    for name, c in obj.cost_functions.items():
        jac, err = c.weighted_jacobians_error()
        assert_blocks_close(err.expand(3, -1).numpy(), g[f"we_{name}"], 1e-12, f"{name} error")
        if not isinstance(c, th.Difference):   # (Difference.error() on SE2 is the HIP kernels', as before)
            assert_blocks_close(c.weighted_error().expand(3, -1).numpy(), g[f"we_{name}"], 1e-12, f"{name} weighted_error")
        assert len(jac) == len(c.optim_vars())
        for s, j in enumerate(jac):
            assert_blocks_close(j.expand(3, -1, -1).numpy(), g[f"wj_{name}_{s}"], 1e-12, f"{name} block {s}")


def test_fixtures_cover_the_cases():
    covered = set()
    for fixture in FIXTURES:
        covered |= classify(load_golden(fixture))
    assert covered == ALL_CASES
    # a moving-frame residual rotation of exactly 0 (Taylor branch) and the relative rotations near +-pi are in the recorded errors
    g = load_golden(FIXTURES[1])
    assert (g["we_mf_between_1_3"][:2, 2] == [0.0, g["we_mf_between_1_3"][1, 2]]).all() and 0 < abs(g["we_mf_between_1_3"][1, 2]) < 1e-6


def _lm(th, g, kernels, device="cpu", **okw):
    obj, leaves, _ = build(th, g, device=device, grad=bool(okw.get("backward_mode")) and not okw.pop("no_leaves", False))
    opt = th.LevenbergMarquardt(obj, linearization_kwargs=dict(kernels=kernels) if kernels is not None else {}, **LM_KW)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)   # (info.state_history is kept in the default dtype, as the reference keeps it)
    try:
        sol, info = th.TheseusLayer(opt).forward(None, optimizer_kwargs=dict(damping=LM_DAMPING, **okw))
    finally:
        torch.set_default_dtype(old)
    return obj, opt, leaves, sol, info


def check_iterates(g, info, names):
    """tests/test_traj2_host.py's check_iterates and its bound (rtol 1e-8, atol 1e-10; the error history at rtol 1e-6)"""
    got = torch.cat([info.state_history[k] for k in names], dim=1).permute(2, 0, 1).double().numpy()
    np.testing.assert_allclose(got, g["lm_iterates"], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(info.err_history.numpy(), g["lm_err_history"], rtol=1e-6)


def check_implicit_gradients(g, leaves, sol, names):
    """tests/test_traj2_host.py's check_implicit_gradients and its bound (1e-6 of the gradient's largest entry)"""
    final = state_of(sol, names)
    np.testing.assert_allclose(final.detach().cpu().numpy(), g["implicit_final"], rtol=1e-8, atol=1e-10)
    (final ** 2).sum().backward()
    for k, leaf in leaves.items():
        want = g[f"grad_{k}"]
        assert np.abs(want).max() > 0
        np.testing.assert_allclose(leaf.grad.cpu().numpy(), want, rtol=0, atol=1e-6 * np.abs(want).max(), err_msg=k)


@pytest.mark.parametrize("fixture", FIXTURES)
def test_packed_planar_pushing_on_the_stand_in_kernels(fixture):
    """The packer's term table, decoded by the numpy stand-in of the two kernels: linearization, LM iterates, implicit gradients."""
    import theseus_amd as th
    from tests.push2_oracle_kernels import Push2OracleKernels
    g = load_golden(fixture)
    K = Push2OracleKernels()
    obj, _, _ = build(th, g)
    lin = th.HipLinearization(obj, kernels=K)
    assert type(lin.packed).__name__ == "PackedPlanarPushing" and lin.packed.n == 36 and lin.packed.ld == 64
    lin.linearize()
    assert K.calls["push2_eval"] == 1
    assert_blocks_close(torch.tril(lin.AtA).numpy(), np.tril(g["AtA"]), 1e-12, "AtA")
    assert_blocks_close(lin.Atb.squeeze(2).numpy(), g["Atb"], 1e-12, "Atb")
    assert_blocks_close(obj.error_metric().numpy(), g["error_metric"], 1e-12, "error metric")
    assert K.calls["push2_error"] == 1
    assert_blocks_close(lin.packed.error_vector().numpy(), g["error"], 1e-12, "error vector")
    A, b = lin.packed.dense_A_b()
    v = torch.randn(3, 36, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    np.testing.assert_allclose(lin.Av(v).numpy(), (A @ v.unsqueeze(2)).squeeze(2).numpy(), rtol=1e-12, atol=1e-12)
    with torch.no_grad():
        _, opt, _, _, info = _lm(th, g, K, track_err_history=True, track_state_history=True)
    check_iterates(g, info, g["var_order"].tolist())
    _, _, leaves, sol, _ = _lm(th, g, K, backward_mode="implicit")
    check_implicit_gradients(g, leaves, sol, g["var_order"].tolist())


def test_the_torch_class_path_of_the_packer_equals_the_fused_one():
    """``fused = False`` (the baseline of tools/bench_push2.py): the same packed class on the torch classes"""
    import theseus_amd as th
    from tests.push2_oracle_kernels import Push2OracleKernels
    g = load_golden(FIXTURES[1])
    hist = {}
    for fused in (True, False):
        obj, _, _ = build(th, g)
        opt = th.LevenbergMarquardt(obj, linearization_kwargs=dict(kernels=Push2OracleKernels()), **LM_KW)
        opt.linear_solver.linearization.packed.fused = fused
        with torch.no_grad():
            info = opt.optimize(damping=LM_DAMPING, track_err_history=True)
        hist[fused] = info.err_history.numpy()
    np.testing.assert_allclose(hist[False], hist[True], rtol=1e-9)
    np.testing.assert_allclose(hist[False], g["lm_err_history"], rtol=1e-6)


@pytest.mark.parametrize("mode,kw", [("unroll", {}), ("truncated", dict(backward_num_iterations=2))])
def test_unrolled_modes_are_refused_by_name_and_run_under_no_grad(mode, kw):
    import theseus_amd as th
    from tests.push2_oracle_kernels import Push2OracleKernels
    g = load_golden(FIXTURES[0])
    with pytest.raises(NotImplementedError, match=f"backward_mode='{mode}'.*planar pushing"):
        _lm(th, g, Push2OracleKernels(), backward_mode=mode, **kw)
    with torch.no_grad():
        _, _, _, _, info = _lm(th, g, Push2OracleKernels(), backward_mode=mode, track_err_history=True, track_state_history=True, **kw)
    check_iterates(g, info, g["var_order"].tolist())


def test_packed_for_selects_the_family():
    import theseus_amd as th
    from tests.helpers import load_golden as lg
    from tests.oracle_kernels import OracleKernels
    from tests.push2_oracle_kernels import Push2OracleKernels
    from tests.traj2_common import build as build_traj
    from tests.traj2_oracle_kernels import Traj2OracleKernels
    from theseus_amd.packed import UnsupportedObjective, packed_for
    obj, _, _ = build(th, load_golden(FIXTURES[0]))
    K = Push2OracleKernels()
    p = packed_for(obj, K)
    assert type(p).__name__ == "PackedPlanarPushing" and packed_for(obj, K) is p   # (a built instance is reused)
    # an SE2 pose graph, a trajectory objective and a Vector objective keep their families
    dt = torch.float64
    a, b = th.SE2(dtype=dt, name="a"), th.SE2(dtype=dt, name="b")
    pg = th.Objective(dtype=dt)
    pg.add(th.Between(a, b, th.SE2(dtype=dt, name="m"), th.ScaleCostWeight(torch.ones(1, 1, dtype=dt)), name="e"))
    pg.add(th.Difference(a, th.SE2(dtype=dt, name="t"), th.ScaleCostWeight(torch.ones(1, 1, dtype=dt)), name="p"))
    assert type(packed_for(pg, K)).__name__ == "PackedPoseGraph"
    traj, _, _ = build_traj(th, lg("traj2_f64_shared"))
    assert type(packed_for(traj, Traj2OracleKernels())).__name__ == "PackedTrajectory2D"
    v = th.Vector(2, dtype=dt, name="v")
    vec = th.Objective(dtype=dt)
    vec.add(th.AutoDiffCostFunction([v], lambda optim_vars, aux_vars: optim_vars[0].tensor ** 2, 2, name="sq"))
    assert type(packed_for(vec, K)).__name__ == "PackedEuclidean"
    # kernels without the fused evaluation, and a mixed objective: no planar-pushing packer (and no other family takes SE2 + these costs)
    with pytest.raises(UnsupportedObjective):
        packed_for(build(th, load_golden(FIXTURES[0]))[0], OracleKernels())
    mixed, _, _ = build(th, load_golden(FIXTURES[0]))
    mixed.add(th.Difference(v, th.Vector(2, dtype=dt, name="v_target"), th.ScaleCostWeight(torch.ones(1, 1, dtype=dt)), name="v_prior"))
    with pytest.raises(UnsupportedObjective):
        packed_for(mixed, K)


def test_out_of_scope_arguments_and_bad_auxiliaries_are_refused():
    import theseus_amd as th
    from tests.push2_oracle_kernels import Push2OracleKernels
    dt = torch.float64
    a, b = th.SE2(dtype=dt, name="a"), th.SE2(dtype=dt, name="b")
    sdf, origin, w = torch.zeros(1, 4, 5, dtype=dt), torch.zeros(1, 2, dtype=dt), th.ScaleCostWeight(torch.ones(1, 1, dtype=dt))
    with pytest.raises(NotImplementedError, match="huber"):
        th.eb.EffectorObjectContactPlanar(a, b, origin, sdf, 0.25, 0.1, w, use_huber_loss=True)
    with pytest.raises(ValueError, match="SE2"):
        th.eb.QuasiStaticPushingPlanar(a, b, th.SE3(dtype=dt), b, 1.0, w)
    with pytest.raises(ValueError, match="Inconsistent types"):
        th.eb.MovingFrameBetween(a, b, a, b, th.SE3(dtype=dt), w)
    # set_aux_var_at keeps the SDF container current
    c = th.eb.EffectorObjectContactPlanar(a, b, origin, sdf, 0.25, 0.1, w)
    new = th.Variable(torch.ones(1, 4, 5, dtype=dt), name="other_grid")
    c.set_aux_var_at(1, new)
    assert c.sdf_data is new and c.sdf.sdf_data is new and c.aux_vars()[1] is new
    assert float(c.error()[0, 0]) == pytest.approx(0.9)
    # auxiliary tensors of another dtype / a wrong shape
    g = load_golden(FIXTURES[0])
    obj, _, _ = build(th, g)
    lin = th.HipLinearization(obj, kernels=Push2OracleKernels())
    lin.linearize()
    radius, qsp_weight = obj.get_variable("eff_radius"), obj.get_variable("qsp_weight")
    radius.tensor = torch.zeros(1, 1, dtype=torch.float32)   # (assigned, as the reference allows: Variable.update checks the dtype)
    with pytest.raises(RuntimeError, match="auxiliary tensor lives on"):
        lin.linearize()
    radius.tensor = torch.zeros(1, 2, dtype=dt)
    with pytest.raises(ValueError, match="does not fit batch"):
        lin.linearize()
    radius.tensor, qsp_weight.tensor = torch.zeros(1, 1, dtype=dt), torch.ones(1, 2, dtype=dt)
    with pytest.raises(ValueError, match="3-dimensional DiagonalCostWeight"):
        lin.linearize()


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_header_library_and_ctypes_table_agree(lib_path):  # noqa: F811
    from theseus_amd import _lib
    from theseus_amd.pushing import PUSH2_TERM
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "theseus_hip.h")).read(), flags=re.S)
    orders = {"thx_push2_eval": "terms n_terms x V J j_total e lde m B dtype eps stream", "thx_push2_error": "terms n_terms x V err B dtype eps stream"}
    for name in NAMES:
        assert name in declared_symbols() and name in _lib.EXPORTED_SYMBOLS
        assert hasattr(ctypes.CDLL(lib_path), name)
        proto = re.search(name + r"\s*\((.*?)\)\s*;", header, flags=re.S).group(1)
        args = [a.split()[-1].lstrip("*") for a in proto.split(",")]
        assert args == orders[name].split() and len(_lib._SIGNATURES[name]) == len(args)
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert _lib.load().thx_abi_version() == 30 == _lib.ABI_VERSION
    # sizeof(thx_push2_term) and its field offsets against the numpy dtype
    struct = re.search(r"typedef struct \{([^}]*)\} thx_push2_term;", header).group(1)
    fields = re.findall(r"(\w+)(?:\[(\d+)\])?\s*[,;]", struct)
    assert [f for f, _ in fields] == ["kind", "row0", "pose", "rows", "cols", "j_off", "aux", "aux_bstride", "wdim", "pad_"]
    assert PUSH2_TERM.itemsize == 128 and [PUSH2_TERM.fields[k][1] for k in ("kind", "row0", "pose", "rows", "cols", "j_off", "aux",
                                                                            "aux_bstride", "wdim")] == [0, 4, 8, 24, 28, 32, 40, 80, 120]
    assert "push_kernels.hip" in __import__("theseus_amd.build", fromlist=["SOURCES"]).SOURCES
    assert (_lib.PUSH2_QSP, _lib.PUSH2_MFB, _lib.PUSH2_CONTACT, _lib.PUSH2_PRIOR) == tuple(
        int(re.search(rf"#define THX_PUSH2_{k} (\d)", header).group(1)) for k in ("QSP", "MFB", "CONTACT", "PRIOR"))


def test_bad_arguments_are_refused_before_any_launch(lib_path):  # noqa: F811
    from theseus_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    eps = _lib.SE2Eps(1e-6, 1e-3)
    ok = dict(terms=p, n_terms=3, x=p, V=12, J=p, j_total=40, e=p, lde=12, m=12, err=p, B=2, dtype=0, eps=eps, stream=None)
    orders = {"thx_push2_eval": ("terms", "n_terms", "x", "V", "J", "j_total", "e", "lde", "m", "B", "dtype", "eps", "stream"),
              "thx_push2_error": ("terms", "n_terms", "x", "V", "err", "B", "dtype", "eps", "stream")}
    for fname, order in orders.items():
        f = getattr(lib, fname)

        def refused(needle, **kw):
            a = dict(ok, **kw)
            rc = f(*[a[k] for k in order])
            return rc == -1 and needle in lib.thx_last_error() and fname.encode() in lib.thx_last_error()
        for name in order:
            if isinstance(ok[name], ctypes.c_void_p):
                assert refused(b"null pointer", **{name: None}), (fname, name)
                assert refused(b"aligned", **{name: ctypes.c_void_p(4098)}), (fname, name)
        assert refused(b"null pointer", eps=None)
        assert refused(b"dtype", dtype=7) and refused(b"dtype", dtype=-1)
        assert refused(b"n_terms", n_terms=0) and refused(b"batch", B=0) and refused(b"batch", B=-3)
        assert refused(b"V < 1", V=0)
        assert refused(b"aligned", x=ctypes.c_void_p(4104)) and refused(b"aligned", x=ctypes.c_void_p(4112), dtype=1)   # one record
    f = lib.thx_push2_eval
    assert f(p, 3, p, 12, p, 40, p, 11, 12, 2, 0, eps, None) == -1 and b"lde < m" in lib.thx_last_error()
    assert f(p, 3, p, 12, p, 2, p, 12, 12, 2, 0, eps, None) == -1 and b"j_total" in lib.thx_last_error()
    assert f(p, 3, p, 12, ctypes.c_void_p(4100), 40, p, 12, 12, 2, 1, eps, None) == -1 and b"aligned" in lib.thx_last_error()
    assert f(p, 2 ** 31 - 1, p, 12, p, 40, p, 12, 12, 2 ** 31 - 1, 0, eps, None) == -1 and b"grid limit" in lib.thx_last_error()


def test_cpu_tensors_are_refused_by_the_binding(lib_path):  # noqa: F811
    import theseus_amd as th
    K = th.HipKernels()
    x = torch.zeros(2, 3, 4, dtype=torch.float64)
    table = torch.zeros(128, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="HIP device"):
        K.push2_eval(table, 1, x, torch.zeros(27, dtype=torch.float64), 9, torch.zeros(3, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="HIP device"):
        K.push2_error(table, 1, x, torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"\(V, B, 4\)"):
        K.push2_error(table, 1, x[:, :, :3], torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="do not fit"):
        K.push2_error(table, 1, x, torch.zeros(2, dtype=torch.float64))


def test_argument_checks_under_the_host_sanitizers(tmp_path):
    """A stand-alone program (tests/hostmath/push2_args.cpp) linked with csrc/push_kernels.hip alone, host code built with
    AddressSanitizer + UndefinedBehaviorSanitizer: every bad call is refused, nothing is launched, the sanitizers stay quiet."""
    from theseus_amd import build as b
    exe = str(tmp_path / "push2_args")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wno-unused-value", "-Wno-pass-failed",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "include"), "-I" + b.CSRC, os.path.join(ROOT, "tests", "hostmath", "push2_args.cpp"),
                    os.path.join(b.CSRC, "push_kernels.hip"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "ALL REFUSED" in run.stdout, run.stdout + run.stderr


def test_sliced_auxiliaries_are_read_in_place():
    """The (B, 4) slices of a batched measurement / motion-capture tensor (non-contiguous for B > 1) go into the term table with
    their own batch stride: no private copy, so the table is built once and an in-place edit of the batched tensor is seen."""
    import theseus_amd as th
    from tests.push2_oracle_kernels import Push2OracleKernels
    g = load_golden(FIXTURES[1])
    obj, leaves, _ = build(th, g)
    assert not leaves["meas"][:, 1].is_contiguous()
    lin = th.HipLinearization(obj, kernels=Push2OracleKernels())
    lin.linearize()
    packed = lin.packed
    table, key = packed._table, packed._aux_key
    assert key is not None
    assert_blocks_close(lin.Atb.squeeze(2).numpy(), g["Atb"], 1e-12, "Atb")
    obj.error_metric()
    packed.sync(deep=True)
    assert packed._table is table
    with torch.no_grad():
        leaves["meas"][:, 1, :2] += 0.05
    before = lin.Atb.clone()
    lin.linearize()
    assert packed._table is table and float((lin.Atb - before).abs().max()) > 1e-3
