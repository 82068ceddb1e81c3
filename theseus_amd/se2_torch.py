"""Differentiable SE2 arithmetic in torch: plain functions on (B|1, 4) = [x, y, cos, sin] tensors, tangent [u_x, u_y, theta], right
perturbations -- written from the closed forms of theseus/geometry/se2.py (:130-150 theta / xy, :165-229 log + Jlog, :239-300 exp +
Jexp, :309-339 adjoint / compose / inverse, :399-432 transform_to), so2.py (unrotate) and lie_group.py (:125-136 between, :162-195
compose / inverse / local Jacobians), in the reference's operation order and with its Taylor switches.  The thresholds are the ones
the HIP kernels get (``kernels.se2_eps``).  They run wherever the tensors live and autograd goes through them: the cost classes of
theseus_amd/embodied.py (planar pushing) are built on them, and they are the differentiable twin of csrc/lie_se2.cuh for the
implicit step of PackedPlanarPushing.  Jacobians are (B, rows, 3 | 2) dense tensors assembled with ``stack`` (no in-place writes).
"""
import torch


def _thresholds(dtype):
    from .kernels import se2_eps
    e = se2_eps(dtype)
    return e.near_zero, e.d_near_zero


def _mat(rows):
    """[[a, b, ...], ...] of (B,) tensors -> (B, r, c)"""
    return torch.stack([torch.stack(r, dim=1) for r in rows], dim=1)


def _bc(*ts):
    return torch.broadcast_tensors(*ts)


def exp(xi: torch.Tensor, jac: bool = False):
    """(B, 3) -> (B, 4) [, Jexp (B, 3, 3)]"""
    ux, uy, th = xi[:, 0], xi[:, 1], xi[:, 2]
    cosine, sine = th.cos(), th.sin()
    small = th.abs() < _thresholds(xi.dtype)[0]
    one = torch.ones((), dtype=xi.dtype, device=xi.device)
    th2, th3 = th ** 2, th ** 3
    th_nz = torch.where(small, one, th)
    sbt = torch.where(small, 1 - th2 / 6, sine / th_nz)
    cm1bt = torch.where(small, -th / 2 + th3 / 24, (cosine - 1) / th_nz)
    X = torch.stack([sbt * ux + cm1bt * uy, sbt * uy - cm1bt * ux, cosine, sine], dim=1)
    if not jac:
        return X
    th2_nz = torch.where(small, one, th2)
    tms = torch.where(small, th - th3 / 120, (th - sine) / th2_nz)
    cm1bt2 = torch.where(small, -0.5 + th2 / 24, (cosine - 1) / th2_nz)
    zero, ones = torch.zeros_like(th), torch.ones_like(th)
    J = _mat([[sbt, -cm1bt, tms * ux + cm1bt2 * uy], [cm1bt, sbt, tms * uy - cm1bt2 * ux], [zero, zero, ones]])
    return X, J


def theta(X: torch.Tensor, jac: bool = False):
    """(B, 1) rotation angle [, its (B, 1, 3) Jacobian [0, 0, 1]]"""
    th = torch.atan2(X[:, 3], X[:, 2]).unsqueeze(1)
    if not jac:
        return th
    J = torch.zeros(X.shape[0], 1, 3, dtype=X.dtype, device=X.device)
    J[:, 0, 2] = 1
    return th, J


def log(X: torch.Tensor, jac: bool = False):
    """(B, 4) -> (B, 3) [, Jlog (B, 3, 3)]"""
    x, y, cosine, sine = X[:, 0], X[:, 1], X[:, 2], X[:, 3]
    th = torch.atan2(sine, cosine)
    nz, dnz = _thresholds(X.dtype)
    small = th.abs() < nz
    one = torch.ones((), dtype=X.dtype, device=X.device)
    sine_nz = torch.where(small, one, sine)
    h = 0.5 * (1 + cosine) * torch.where(small, 1 + sine ** 2 / 6, th / sine_nz)
    ht = 0.5 * th
    ux = h * x + ht * y
    uy = h * y - ht * x
    xi = torch.stack([ux, uy, th], dim=1)
    if not jac:
        return xi
    th2 = th ** 2
    th3 = th * th2
    dsmall = th.abs() < dnz
    th_nz = torch.where(dsmall, one, th)
    omc_nz = torch.where(dsmall, one, 1 - cosine)
    a = torch.where(dsmall, 1 - th2 / 12.0, ht * sine / omc_nz)
    k = torch.where(dsmall, th / 12.0 + th3 / 720.0, 1.0 / th_nz - 0.5 * sine / omc_nz)
    zero, ones = torch.zeros_like(th), torch.ones_like(th)
    J = _mat([[a, -ht, k * ux + 0.5 * uy], [ht, a, k * uy - 0.5 * ux], [zero, zero, ones]])
    return xi, J


def adjoint(X: torch.Tensor) -> torch.Tensor:
    x, y, c, s = X[:, 0], X[:, 1], X[:, 2], X[:, 3]
    zero, ones = torch.zeros_like(x), torch.ones_like(x)
    return _mat([[c, -s, y], [s, c, -x], [zero, zero, ones]])


def inverse(X: torch.Tensor, jac: bool = False):
    """X^-1 [, its Jacobian -Ad(X)]"""
    x, y, c, s = X[:, 0], X[:, 1], X[:, 2], X[:, 3]
    nx, ny, ns = -x, -y, -s
    Y = torch.stack([c * nx - ns * ny, ns * nx + c * ny, c, ns], dim=1)   # R^-1 (-t)
    return (Y, -adjoint(X)) if jac else Y


def compose(A: torch.Tensor, B: torch.Tensor, jac: bool = False):
    """A B [, (Ad(B^-1), I)]"""
    A, B = _bc(A, B)
    ax, ay, ac, as_ = A[:, 0], A[:, 1], A[:, 2], A[:, 3]
    bx, by, bc, bs = B[:, 0], B[:, 1], B[:, 2], B[:, 3]
    Z = torch.stack([ax + (ac * bx - as_ * by), ay + (as_ * bx + ac * by), ac * bc - as_ * bs, as_ * bc + ac * bs], dim=1)
    if not jac:
        return Z
    eye = torch.eye(3, dtype=A.dtype, device=A.device).expand(A.shape[0], 3, 3)
    return Z, (adjoint(inverse(B)), eye)


def between(A: torch.Tensor, B: torch.Tensor, jac: bool = False):
    """A^-1 B [, (Ad(B^-1) (-Ad(A)) , I)] (lie_group.py:125-136)"""
    Ai = inverse(A)
    if not jac:
        return compose(Ai, B)
    D, (J0, J1) = compose(Ai, B, jac=True)
    return D, (J0 @ -adjoint(A).expand_as(J0), J1)


def local(A: torch.Tensor, B: torch.Tensor, jac: bool = False):
    """log(A^-1 B) [, (-Ad((A^-1 B)^-1) Jlog, Jlog)] (lie_group.py:180-195)"""
    D = between(A, B)
    if not jac:
        return log(D)
    xi, Jl = log(D, jac=True)
    return xi, (-adjoint(inverse(D)) @ Jl, Jl)


def retract(X: torch.Tensor, delta: torch.Tensor) -> torch.Tensor:
    return compose(X, exp(delta))


def xy(X: torch.Tensor, jac: bool = False):
    """translation (B, 2) [, (B, 2, 3) = [R, 0]]"""
    p = X[:, :2]
    if not jac:
        return p
    c, s = X[:, 2], X[:, 3]
    zero = torch.zeros_like(c)
    return p, _mat([[c, -s, zero], [s, c, zero]])


def unrotate(R: torch.Tensor, p: torch.Tensor, jac: bool = False):
    """R^T p for R (B, 2) = [cos, sin] [, (d/d angle (B, 2, 1), d/d p (B, 2, 2) = R^T)] (so2.py: unrotate)"""
    R, p = _bc(R, p)
    c, s = R[:, 0], R[:, 1]
    ns = -s
    px, py = p[:, 0], p[:, 1]
    rx, ry = c * px - ns * py, ns * px + c * py
    ret = torch.stack([rx, ry], dim=1)
    if not jac:
        return ret
    return ret, (torch.stack([ry, -rx], dim=1).unsqueeze(2), _mat([[c, s], [-s, c]]))


def transform_to(X: torch.Tensor, p: torch.Tensor, jac: bool = False):
    """R^T (p - t) [, (d/d X (B, 2, 3), d/d p (B, 2, 2))] (se2.py:399-432)"""
    X, _ = _bc(X, torch.cat([p, p], dim=1))
    c, s = X[:, 2], X[:, 3]
    ns = -s
    tmp = p - X[:, :2]
    tx, ty = tmp[:, 0], tmp[:, 1]
    rx, ry = c * tx - ns * ty, ns * tx + c * ty
    ret = torch.stack([rx, ry], dim=1)
    if not jac:
        return ret
    zero, m1 = torch.zeros_like(rx), -torch.ones_like(rx)
    return ret, (_mat([[m1, zero, ry], [zero, m1, -rx]]), _mat([[c, s], [-s, c]]))
