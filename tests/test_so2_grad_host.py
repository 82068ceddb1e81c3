"""-m "not gpu": gradients of SO2 pose graphs (th.Between / th.Difference on th.SO2) without a GPU.

* theseus_amd's own loop with the TEST stand-in kernels: backward_mode "implicit" (plain and robust costs), "unroll" and "truncated"
  against the gradients the REAL reference recorded (tests/golden/pgso2_f64_*.npz, tools/gen_golden_so2_grad.py);
* the reference's own loop with the plugin underneath (``reference``: needs the reference importable);
* the device maths of theseus_amd/csrc/vjp_so2.cuh (thx_pgso2_vjp, thx_pgso2_unroll_vjp, thx_so2_retract_vjp), compiled for the host
  (tests/hostmath/so2math.cpp over the tests/hostmath shim), against torch autograd through oracle/lie_so2.py + oracle/pose_graph.py
  -- every loss code, ellipsoidal damping on and off, angles near 0 and near +-pi, records off the unit circle."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import lie_so2
from oracle.gen_golden import REF as REFERENCE_ROOT
from oracle import pose_graph as opg
from tests.conftest import ROOT
from tests.helpers import load_golden
from tests import so2_grad_common as so2g

UNROLLED_TAGS = ["gn_unroll", "lm_trunc", "lm_ellips_unroll"]
IMPLICIT = [("pgso2_f64_implicit", False), ("pgso2_f64_robust_implicit", True)]


def _standin():
    from tests.oracle_kernels import OracleKernels
    return dict(linearization_kwargs=dict(kernels=OracleKernels()))


# ---- theseus_amd's own loop -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,robust", IMPLICIT)
def test_implicit_gradients_of_an_so2_graph_match_reference(name, robust):
    import theseus_amd as th
    g = load_golden(name)
    final, loss, grads, info = so2g.run(th, g, robust=robust, optimizer_kwargs=_standin())
    so2g.check_implicit(g, final, loss, grads)
    assert info.iters_done == 6


@pytest.mark.parametrize("tag", UNROLLED_TAGS)
def test_unrolled_gradients_of_an_so2_graph_match_reference(tag):
    import theseus_amd as th
    g = load_golden("pgso2_f64_unrolled")
    so2g.check_unrolled(g, tag, *so2g.run(th, g, tag=tag, optimizer_kwargs=_standin()))


def test_trust_region_with_unrolled_gradients_stays_refused_for_so2():
    """The one refusal SO2 shares with every group: Dogleg's step reads Av() outside autograd."""
    import theseus_amd as th
    g = load_golden("pgso2_f64_implicit")
    obj, _ = so2g.build(th, g)
    dog = th.Dogleg(obj, max_iterations=2, **_standin())
    with pytest.raises(NotImplementedError, match="trust-region"):
        th.TheseusLayer(dog).forward(None, optimizer_kwargs=dict(backward_mode="unroll"))


def test_vjp_entry_points_are_chosen_by_the_exact_record_shape():
    from theseus_amd.kernels import vjp_group
    for shape, grp in (((3, 4), "SE3"), ((3, 3), "SO3"), ((4,), "SE2"), ((2,), "SO2")):
        assert vjp_group(torch.zeros(5, 2, *shape)) == grp
    for shape in ((3,), (1,), (2, 2), (4, 4)):
        with pytest.raises(ValueError, match="no VJP kernel"):
            vjp_group(torch.zeros(5, 2, *shape))


# ---- the reference's loop with the plugin -------------------------------------------------------------------------------------------
REF = os.environ.get("THX_REFERENCE_ROOT", REFERENCE_ROOT)
needs_reference = pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference")


@pytest.fixture(scope="module")
def ref():
    for p in (os.path.join(ROOT, "oracle", "stubs"), REF, REF + "/torchlie", REF + "/torchkin"):
        if p not in sys.path:
            sys.path.append(p)   # appended: the reference has its own top-level ``tests`` package
    import warnings
    warnings.filterwarnings("ignore")
    import theseus as th
    import theseus_amd.plugin as thp
    return th, thp


def _plugin(thp):
    return dict(linear_solver_cls=thp.HipCholeskySolver, linearization_cls=thp.HipLinearization, vectorize=True, **_standin())


@pytest.mark.reference
@needs_reference
@pytest.mark.parametrize("name,robust", IMPLICIT)
def test_implicit_gradients_through_the_reference_loop_and_the_plugin(ref, name, robust):
    """_HipRetract / _FusedAtb (thx_so2_retract_vjp / thx_pgso2_vjp behind the stand-in) under the REAL TheseusLayer."""
    th, thp = ref
    g = load_golden(name)
    final, loss, grads, _ = so2g.run(th, g, robust=robust, optimizer_kwargs=_plugin(thp))
    so2g.check_implicit(g, final, loss, grads)


@pytest.mark.reference
@needs_reference
@pytest.mark.parametrize("tag", UNROLLED_TAGS)
def test_unrolled_gradients_through_the_reference_loop_and_the_plugin(ref, tag):
    """_FusedUnrolledSolve (thx_pgso2_unroll_vjp behind the stand-in) under the REAL loop; retraction and error in between are the
    reference's own differentiable ops."""
    th, thp = ref
    g = load_golden("pgso2_f64_unrolled")
    so2g.check_unrolled(g, tag, *so2g.run(th, g, tag=tag, optimizer_kwargs=_plugin(thp)))


# ---- vjp_so2.cuh on the host ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def so2math(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("so2math") / "libso2math.so")
    src = os.path.join(ROOT, "tests", "hostmath")
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", f"-I{src}", f"-I{ROOT}/theseus_amd/csrc", "-Wno-unknown-pragmas",
                    os.path.join(src, "so2math.cpp"), "-o", out], check=True)
    lib = ctypes.CDLL(out)
    dp, d, i = ctypes.POINTER(ctypes.c_double), ctypes.c_double, ctypes.c_int
    lib.so2_implicit_vjp.argtypes = [dp, dp, d, d, i, d, dp]
    lib.so2_unroll.argtypes = [i, dp, dp, dp, d, d, d, d, d, d, i, d, dp]
    lib.so2_retract.argtypes = [dp, dp, d]
    lib.so2_retract.restype = d
    return lib


def _ptr(a):
    return np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))


LOSSES = [(0, None), (1, "welsch"), (2, "huber"), (5, "welsch+flatten"), (6, "huber+flatten"), (3, "hinge"), (7, "hinge+flatten"),
          (8, "gm"), (12, "gm+flatten")]   # (THX_LOSS_* code, oracle spec)
# angle of E = Z^-1 D: generic, near 0, just inside +pi and just inside -pi (either side of the atan2 branch cut), large
ANGLES = [0.7, 1e-4, np.pi - 1e-3, -np.pi + 1e-3, 2.9]
SO2 = opg.GROUPS["SO2"]


def _rec(theta, scale=1.0):
    """A raw record [cos, sin] * scale (scale != 1: off the unit circle -- never re-normalised)."""
    return lie_so2.so2_exp(torch.tensor([[theta]], dtype=torch.float64))[0] * scale


def _case(seed, angle):
    gen = torch.Generator().manual_seed(seed)
    u = lambda lo, hi: float(lo + (hi - lo) * torch.rand(1, dtype=torch.float64, generator=gen))  # noqa: E731
    Xi, Xj = _rec(u(-np.pi, np.pi), u(0.8, 1.25)), _rec(u(-np.pi, np.pi), u(0.8, 1.25))
    D = SO2.compose(SO2.inverse(Xi), Xj)
    Dth = float(lie_so2.so2_log(D))
    Z = _rec(Dth - angle, u(0.8, 1.25))           # E = Z^-1 D has angle ~ ``angle`` (off-manifold records included)
    s = u(0.5, 1.5)
    wi, wj, di, dj = (float(torch.randn(1, dtype=torch.float64, generator=gen)) for _ in range(4))
    return Xi, Xj, Z, s, wi, wj, di, dj


def _robust(Js, e, spec, lr):
    if spec is None:
        return Js, e
    Jr, er = opg.robust_rescale([J.view(1, 1, 1, 1) for J in Js], e.view(1, 1, 1), spec if "+" not in spec else [spec], lr)
    return [J.view(1, 1) for J in Jr], er.view(1)


def _log_radius(x0, seed):
    # (near the squared error, so that Huber's / Hinge's knee and Welsch's decay are exercised)
    return torch.tensor([[np.log(max(x0, 1e-12)) - 0.3 + 0.2 * seed]], dtype=torch.float64)


def _check(got, leaves, names, what):
    for (name, sl), leaf in zip(names, leaves):
        if leaf.grad is None:           # (a plain cost does not depend on log_loss_radius)
            assert name == "log_radius" and got[sl].tolist() == [0.0], what
            continue
        want = leaf.grad.numpy().reshape(-1)
        np.testing.assert_allclose(got[sl], want, rtol=0, atol=1e-11 * max(1.0, np.abs(want).max()), err_msg=f"{what} {name}")


@pytest.mark.parametrize("code,spec", LOSSES)
@pytest.mark.parametrize("angle", ANGLES)
@pytest.mark.parametrize("seed", [0, 1])
def test_implicit_cost_vjp_matches_autograd_through_the_oracle(so2math, seed, angle, code, spec):
    """thx_pgso2_vjp's per-cost maths: gradient of phi = w^T g = -(J_i w_i + J_j w_j) e (robust: rescaled) w.r.t. the measurement /
    target (raw entries), the weight and log_loss_radius, for a Between cost and a Difference prior."""
    Xi, Xj, Z, s, wi, wj, _, _ = _case(seed, angle)
    sw = torch.tensor([s], dtype=torch.float64)
    # ---- Between ----
    with torch.no_grad():
        x0 = float((opg.between_jac_err(Xi, Xj, Z, sw, SO2)[2] ** 2).sum())
    leaves = [t.clone().requires_grad_(True) for t in (Z, sw, _log_radius(x0, seed))]
    J0, J1, e = opg.between_jac_err(Xi, Xj, leaves[0], leaves[1], SO2)
    (J0, J1), e = _robust([J0, J1], e, spec, leaves[2])
    (-((J0 * wi + J1 * wj).view(1) * e).sum()).backward()
    C = SO2.compose(SO2.inverse(Xi), Xj)
    out = np.zeros(4)
    so2math.so2_implicit_vjp(_ptr(Z), _ptr(C), wj - wi, s, code, leaves[2].item(), _ptr(out))
    _check(out, leaves, (("Z", slice(0, 2)), ("s", slice(2, 3)), ("log_radius", slice(3, 4))), "between")
    # ---- Difference / Local prior: e = log(T^-1 X) ----
    X, T = Xj, Z
    with torch.no_grad():
        x0 = float((opg.local_jac_err(T, X, sw, SO2)[1] ** 2).sum())
    leaves = [t.clone().requires_grad_(True) for t in (T, sw, _log_radius(x0, seed))]
    J, e = opg.local_jac_err(leaves[0], X, leaves[1], SO2)
    (J,), e = _robust([J], e, spec, leaves[2])
    (-((J * wj).view(1) * e).sum()).backward()
    out = np.zeros(4)
    so2math.so2_implicit_vjp(_ptr(T), _ptr(X), wj, s, code, leaves[2].item(), _ptr(out))
    _check(out, leaves, (("T", slice(0, 2)), ("s", slice(2, 3)), ("log_radius", slice(3, 4))), "prior")


@pytest.mark.parametrize("code,spec", LOSSES)
@pytest.mark.parametrize("lam", [0.0, 0.37])     # (> 0: ellipsoidal damping's term -lambda sum_i w_i delta_i H_ii)
@pytest.mark.parametrize("angle", ANGLES)
def test_unrolled_cost_vjp_matches_autograd_through_the_oracle(so2math, angle, lam, code, spec):
    """thx_pgso2_unroll_vjp's per-cost maths: gradient of phi = -(J w)(e + J delta) - lambda sum_i w_i delta_i (J^T J)_ii w.r.t. both
    poses, the measurement / target, the weight and log_loss_radius."""
    Xi, Xj, Z, s, wi, wj, di, dj = _case(3, angle)
    sw = torch.tensor([s], dtype=torch.float64)
    # ---- Between ----
    with torch.no_grad():
        x0 = float((opg.between_jac_err(Xi, Xj, Z, sw, SO2)[2] ** 2).sum())
    leaves = [t.clone().requires_grad_(True) for t in (Xi, Xj, Z, sw, _log_radius(x0, 0))]
    J0, J1, e = opg.between_jac_err(*leaves[:4], SO2)
    (J0, J1), e = _robust([J0, J1], e, spec, leaves[4])
    J0, J1 = J0.view(1), J1.view(1)
    phi = -((J0 * wi + J1 * wj) * (e + J0 * di + J1 * dj)).sum() - lam * (J0 ** 2 * wi * di + J1 ** 2 * wj * dj).sum()
    phi.backward()
    out = np.zeros(8)
    so2math.so2_unroll(1, _ptr(Xi), _ptr(Xj), _ptr(Z), s, wi, wj, di, dj, lam, code, leaves[4].item(), _ptr(out))
    _check(out, leaves, (("Xi", slice(0, 2)), ("Xj", slice(2, 4)), ("Z", slice(4, 6)), ("s", slice(6, 7)), ("log_radius", slice(7, 8))),
           "between")
    # ---- Difference / Local prior ----
    X, T = Xj, Z
    with torch.no_grad():
        x0 = float((opg.local_jac_err(T, X, sw, SO2)[1] ** 2).sum())
    leaves = [t.clone().requires_grad_(True) for t in (X, T, sw, _log_radius(x0, 1))]
    J, e = opg.local_jac_err(leaves[1], leaves[0], leaves[2], SO2)
    (J,), e = _robust([J], e, spec, leaves[3])
    J = J.view(1)
    (-((J * wj) * (e + J * dj)).sum() - lam * (J ** 2 * wj * dj).sum()).backward()
    out = np.zeros(8)
    so2math.so2_unroll(0, _ptr(X), _ptr(X), _ptr(T), s, 0.0, wj, 0.0, dj, lam, code, leaves[3].item(), _ptr(out))
    assert out[:2].tolist() == [0.0, 0.0]
    _check(out, leaves, (("X", slice(2, 4)), ("T", slice(4, 6)), ("s", slice(6, 7)), ("log_radius", slice(7, 8))), "prior")


@pytest.mark.parametrize("theta", [0.3, 1e-6, np.pi - 1e-3, -3.5])
@pytest.mark.parametrize("scale", [1.0, 0.8, 1.25])
def test_retract_vjp_matches_autograd_through_the_oracle(so2math, theta, scale):
    """thx_so2_retract_vjp's maths: d/dtheta <G, X exp(theta)> (lie_group.py:197-198 over so2.py's exp and compose)."""
    gen = torch.Generator().manual_seed(7)
    X = _rec(2.2, scale)
    G = torch.randn(2, dtype=torch.float64, generator=gen)
    th_ = torch.tensor([[theta]], dtype=torch.float64, requires_grad=True)
    (lie_so2.so2_retract(X.view(1, 2), th_)[0] * G).sum().backward()
    got = so2math.so2_retract(_ptr(X), _ptr(G), theta)
    assert abs(got - float(th_.grad)) <= 1e-13 * max(1.0, abs(float(th_.grad)))
