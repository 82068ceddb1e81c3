"""Differentiable SE3 arithmetic in torch: plain functions on (B|1, 3, 4) = [R | t] tensors, tangent [v, w], right perturbations --
the counterpart of theseus_amd/se2_torch.py, written from the closed forms of SURVEY.md Appendix A (the ones csrc/lie.cuh holds:
torchlie/functional/so3_impl.py exp / log / Jlog, se3_impl.py exp / log / Jlog / adjoint / compose / inverse) with the reference's
Taylor switches.  The thresholds are the ones the HIP kernels get (``kernels.lie_eps``).  They run wherever the tensors live and
autograd goes through them (plain derivatives of the closed forms; a branch that is not taken never sees a zero denominator or the
square root of zero): the link costs of theseus_amd/kinematics.py are built on them, and they are the differentiable twin of
csrc/kin_kernels.hip.  Matrices are assembled with ``stack`` / ``cat`` (no in-place writes).
"""
import torch


def _thresholds(dtype):
    from .kernels import lie_eps
    e = lie_eps(dtype)
    return e.near_zero, e.d_near_zero, e.near_pi


def _safe_sqrt(x, use):
    """sqrt(x) where ``use`` (and x > 0), else 0 -- with a finite derivative everywhere"""
    ok = use & (x > 0)
    return torch.where(ok, torch.sqrt(torch.where(ok, x, torch.ones_like(x))), torch.zeros_like(x))


def hat(w: torch.Tensor) -> torch.Tensor:
    """(B, 3) -> (B, 3, 3) cross-product matrices"""
    z = torch.zeros_like(w[:, 0])
    return torch.stack([torch.stack([z, -w[:, 2], w[:, 1]], dim=1), torch.stack([w[:, 2], z, -w[:, 0]], dim=1),
                        torch.stack([-w[:, 1], w[:, 0], z], dim=1)], dim=1)


def _eye(ref):
    return torch.eye(3, dtype=ref.dtype, device=ref.device)


def _outer(a, b):
    return a.unsqueeze(2) * b.unsqueeze(1)


def _exp_coefficients(w):
    nz_eps = _thresholds(w.dtype)[0]
    theta2 = (w * w).sum(1)
    always = torch.ones_like(theta2, dtype=torch.bool)
    theta = _safe_sqrt(theta2, always)
    nz = theta < nz_eps
    one = torch.ones_like(theta)
    theta_nz, theta2_nz = torch.where(nz, one, theta), torch.where(nz, one, theta2)
    cosine = torch.where(nz, 8 / (4 + theta2) - 1, theta.cos())
    sine = theta.sin()
    A = torch.where(nz, 0.5 * cosine + 0.5, sine / theta_nz)
    Bc = torch.where(nz, 0.5 * A, (1 - cosine) / theta2_nz)
    return theta, theta2, nz, theta_nz, theta2_nz, sine, cosine, A, Bc


def so3_exp(w: torch.Tensor) -> torch.Tensor:
    """(B, 3) -> (B, 3, 3):  cos I + A [w]x + B w w^T"""
    *_, cosine, A, Bc = _exp_coefficients(w)
    return cosine.view(-1, 1, 1) * _eye(w) + A.view(-1, 1, 1) * hat(w) + Bc.view(-1, 1, 1) * _outer(w, w)


def exp(xi: torch.Tensor) -> torch.Tensor:
    """(B, 6) -> (B, 3, 4)"""
    v, w = xi[:, :3], xi[:, 3:]
    theta, theta2, nz, theta_nz, theta2_nz, sine, cosine, A, Bc = _exp_coefficients(w)
    R = cosine.view(-1, 1, 1) * _eye(w) + A.view(-1, 1, 1) * hat(w) + Bc.view(-1, 1, 1) * _outer(w, w)
    C = torch.where(nz, 1.0 / 6 - theta2 / 120, (theta - sine) / (theta_nz * theta2_nz))
    wv = (w * v).sum(1, keepdim=True)
    t = A.unsqueeze(1) * v + Bc.unsqueeze(1) * torch.linalg.cross(w, v, dim=1) + C.unsqueeze(1) * (w * wv)
    return torch.cat([R, t.unsqueeze(2)], dim=2)


def _pair(X, Y):
    B = max(X.shape[0], Y.shape[0])
    return X.expand(B, 3, 4), Y.expand(B, 3, 4)


def compose(X: torch.Tensor, Y: torch.Tensor) -> torch.Tensor:
    """[R0 R1 | R0 t1 + t0]"""
    X, Y = _pair(X, Y)
    R = X[:, :, :3] @ Y[:, :, :3]
    t = X[:, :, :3] @ Y[:, :, 3:] + X[:, :, 3:]
    return torch.cat([R, t], dim=2)


def inverse(X: torch.Tensor) -> torch.Tensor:
    """[R^T | -R^T t]"""
    Rt = X[:, :, :3].transpose(1, 2)
    return torch.cat([Rt, -(Rt @ X[:, :, 3:])], dim=2)


def adjoint(X: torch.Tensor) -> torch.Tensor:
    """(B, 6, 6) = [[R, [t]x R], [0, R]]"""
    R = X[:, :, :3]
    top = torch.cat([R, hat(X[:, :, 3]) @ R], dim=2)
    return torch.cat([top, torch.cat([torch.zeros_like(R), R], dim=2)], dim=1)


def _so3_log(R):
    nz_eps, _, npi_eps = _thresholds(R.dtype)
    sa = 0.5 * torch.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], dim=1)
    cosine = 0.5 * (R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] - 1)
    always = torch.ones_like(cosine, dtype=torch.bool)
    sine = _safe_sqrt((sa * sa).sum(1), always)
    theta = torch.atan2(sine, cosine)
    nz, npi = theta < nz_eps, (1 + cosine) <= npi_eps
    nznp = nz | npi
    one = torch.ones_like(theta)
    scale = torch.where(nznp, 1 + sine * sine / 6, theta / torch.where(nznp, one, sine))
    # near pi: the axis from the row / column of the largest diagonal entry
    d = torch.stack([R[:, 0, 0], R[:, 1, 1], R[:, 2, 2]], dim=1)
    m1 = (d[:, 1] > d[:, 0]) & (d[:, 1] > d[:, 2])
    m2 = (d[:, 2] > d[:, 0]) & (d[:, 2] > d[:, 1])
    major = m1.long() + 2 * m2.long()
    rowv = R.gather(1, major.view(-1, 1, 1).expand(-1, 1, 3)).squeeze(1)
    colv = R.gather(2, major.view(-1, 1, 1).expand(-1, 3, 1)).squeeze(2)
    pick = (major.unsqueeze(1) == torch.arange(3, device=R.device)).to(R.dtype)
    sel = 0.5 * (rowv + colv) - pick * cosine.unsqueeze(1)
    nrm = torch.where(npi, _safe_sqrt((sel * sel).sum(1), npi), one)
    sam = (sa * pick).sum(1)
    sgn = torch.where(sam < 0, -one, one)
    w = torch.where(npi.unsqueeze(1), sel / nrm.unsqueeze(1) * (theta * sgn).unsqueeze(1), sa * scale.unsqueeze(1))
    return w, theta, sine, cosine


def log(X: torch.Tensor, jac: bool = False):
    """(B, 3, 4) -> (B, 6) [, Jlog (B, 6, 6) = [[Jr, Jt], [0, Jr]]: what SE3.log_map(jacobians=...) returns]"""
    nz_eps, dnz_eps, _ = _thresholds(X.dtype)
    R, t = X[:, :, :3], X[:, :, 3]
    w, theta, sine, cosine = _so3_log(R)
    nz = theta < nz_eps
    one = torch.ones_like(theta)
    theta2, st, tcm2 = theta * theta, sine * theta, 2 * cosine - 2
    tcm2_nz, theta2_nz = torch.where(nz, one, tcm2), torch.where(nz, one, theta2)
    a = torch.where(nz, 1 - theta2 / 12, -st / tcm2_nz)
    b = torch.where(nz, 1.0 / 12 + theta2 / 720, (st + tcm2) / (theta2_nz * tcm2_nz))
    wt = (w * t).sum(1, keepdim=True)
    v = a.unsqueeze(1) * t - 0.5 * torch.linalg.cross(w, t, dim=1) + b.unsqueeze(1) * (w * wt)
    xi = torch.cat([v, w], dim=1)
    if not jac:
        return xi
    dnz = theta < dnz_eps
    tcm2_d, theta2_d = torch.where(dnz, one, tcm2), torch.where(dnz, one, theta2)
    a2 = torch.where(dnz, 1 - theta2 / 12, -st / tcm2_d)
    b2 = torch.where(dnz, 1.0 / 12 + theta2 / 720, (st + tcm2) / (theta2_d * tcm2_d))
    bw = b2.unsqueeze(1) * w
    eye = _eye(X)
    Jr = _outer(bw, w) + 0.5 * hat(w) + a2.view(-1, 1, 1) * eye
    theta_d = torch.where(dnz, one, theta)
    theta4_nz = theta2_nz * theta2_nz
    cc = torch.where(dnz, -1.0 / 360 - theta2 / 7560, -(2 * tcm2_nz + theta * sine + theta2) / (theta4_nz * tcm2_nz))
    dd = torch.where(dnz, -1.0 / 6 - theta2 / 180, (theta - sine) / (theta_d * tcm2_nz))
    e = (w * v).sum(1)
    Jt = (cc * e).view(-1, 1, 1) * _outer(w, w) + _outer(bw, v) + _outer(v, bw) + (e * dd).view(-1, 1, 1) * eye + 0.5 * hat(v)
    J = torch.cat([torch.cat([Jr, Jt], dim=2), torch.cat([torch.zeros_like(Jr), Jr], dim=2)], dim=1)
    return xi, J


def local(target: torch.Tensor, X: torch.Tensor, jac: bool = False):
    """log(target^-1 X) [, its Jacobian w.r.t. a right perturbation of X: Jlog]"""
    return log(compose(inverse(target), X), jac)


def axis_rotation(axis: torch.Tensor, angle: torch.Tensor) -> torch.Tensor:
    """The rotation by ``angle`` (B,) about the UNIT vector ``axis`` (3,): I + sin [a]x + (1 - cos) [a]x^2 -- no division, no branch"""
    K = hat(axis.view(1, 3))[0]
    return _eye(angle) + angle.sin().view(-1, 1, 1) * K + (1 - angle.cos()).view(-1, 1, 1) * (K @ K)
