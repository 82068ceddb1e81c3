"""TEST-ONLY: the CPU stand-in of tests/oracle_kernels.py extended by the three exports of csrc/trajse2_kernels.hip, restated in numpy
from include/theseus_hip.h (thx_trajse2_term, its layout written out again below) -- it decodes the SAME term table the HIP kernels
read (the pointers are host pointers here), so the packer's table is checked without a GPU.  Written in matrix form from the formulas
of collision.py, double_integrator.py (the weight by an explicit Kronecker product and numpy's Cholesky), motionmodel/misc.py,
local_cost_fn.py and motion_planner.py's goal cost, on the numpy SE2 helpers of tests/push2_oracle_kernels.py; it shares no code with
the torch classes of theseus_amd/embodied.py, with theseus_amd/se2_torch.py or with theseus_amd/planning_se2.py."""
import numpy as np
import torch

from tests.oracle_kernels import OracleKernels
from tests.push2_oracle_kernels import _aux, adj, inv, log_jlog, mul, rot, sdf_lookup
from theseus_amd.kernels import se2_eps

TERM = np.dtype([("kind", "<i4"), ("row0", "<i4"), ("var", "<i4", (4,)), ("rows", "<i4"), ("cols", "<i4"), ("j_off", "<i8"),
                 ("aux", "<u8", (5,)), ("aux_bstride", "<i8", (5,)), ("wdim", "<i4"), ("pad", "<i4")])
COLLISION, GP, NONHOLONOMIC, HINGE, PRIOR_SE2, PRIOR_VEC, PRIOR_XY = range(7)
DIM = {COLLISION: 1, GP: 6, NONHOLONOMIC: 1, HINGE: 3, PRIOR_SE2: 3, PRIOR_VEC: 3, PRIOR_XY: 2}
NVARS = {COLLISION: 1, GP: 4, NONHOLONOMIC: 2, HINGE: 1, PRIOR_SE2: 1, PRIOR_VEC: 1, PRIOR_XY: 1}


def _weights(term, k, B, dim, np_dtype):
    return np.broadcast_to(_aux(term, k, B, int(term["wdim"]), np_dtype), (B, dim)).astype(np.float64)


def _diag(w):
    return np.einsum("bi,ij->bij", w, np.eye(w.shape[1]))


def gp_weight(dt, Q):
    """U (B, 6, 6) with U^T U = W^T's lower triangle completed symmetrically, W = M (x) Qc_inv: numpy's Cholesky of W^T, transposed"""
    U = np.zeros((len(dt), 6, 6))
    for b in range(len(dt)):
        M = np.array([[12.0 / dt[b] ** 3, -6.0 / dt[b] ** 2], [-6.0 / dt[b] ** 2, 4.0 / dt[b]]])
        U[b] = np.linalg.cholesky(np.kron(M, Q[b]).T).T
    return U


def _term(term, x, B, np_dtype):
    """-> (weighted error (B, dim), [weighted Jacobian blocks (B, dim, 3)])"""
    kind = int(term["kind"])
    P = [x[int(v)].astype(np.float64) for v in term["var"][:NVARS[kind]]]
    aux = lambda k, per: np.broadcast_to(_aux(term, k, B, per, np_dtype), (B, per)).astype(np.float64)  # noqa: E731
    if kind == COLLISION:
        R, C = int(term["rows"]), int(term["cols"])
        sdf = np.broadcast_to(_aux(term, 0, B, R * C, np_dtype), (B, R * C)).reshape(B, R, C).astype(np.float64)
        o, cell, eps, w = aux(1, 2), aux(2, 1), aux(3, 1), aux(4, 1)
        d, grad = sdf_lookup(sdf, o, cell[:, 0], P[0][:, :2])
        Jxy = np.zeros((B, 2, 3))
        Jxy[:, :, :2] = rot(P[0])
        J = -(grad[:, None, :] @ Jxy)
        J[d > eps[:, 0]] = 0.0
        return np.maximum(eps[:, 0] - d, 0.0)[:, None] * w, [J * w[:, :, None]]
    if kind == GP:
        dt, dtw, Q = aux(0, 1), aux(1, 1)[:, 0], aux(2, 9).reshape(B, 3, 3)
        U = gp_weight(dtw, Q)
        p1, v1, p2, v2 = P
        D = mul(inv(p1), p2)
        xi, Jl = log_jlog(D, np_dtype)
        J0 = -(Jl @ adj(inv(D)))
        r = np.concatenate([xi - dt * v1[:, :3], v2[:, :3] - v1[:, :3]], axis=1)
        eye, zero = np.broadcast_to(np.eye(3), (B, 3, 3)), np.zeros((B, 3, 3))
        stack = lambda a, b: np.concatenate([a, b], axis=1)  # noqa: E731
        blocks = [stack(J0, zero), stack(-dt[:, :, None] * eye, -eye), stack(Jl, zero), stack(zero, eye)]
        return np.einsum("bij,bj->bi", U, r), [U @ blk for blk in blocks]
    if kind == NONHOLONOMIC:
        w = aux(0, 1)
        Jv = np.zeros((B, 1, 3))
        Jv[:, 0, 1] = w[:, 0]
        return P[1][:, 1:2] * w, [np.zeros((B, 1, 3)), Jv]
    if kind == HINGE:
        down, up, thr, w = aux(0, 3), aux(1, 3), aux(2, 3), _weights(term, 3, B, 3, np_dtype)
        v, lo, hi = P[0][:, :3], down + thr, up - thr
        err = np.where(v > hi, v - hi, np.where(v < lo, lo - v, 0.0))
        sgn = np.where(v > hi, 1.0, np.where(v < lo, -1.0, 0.0))
        return err * w, [_diag(sgn * w)]
    if kind == PRIOR_SE2:
        target, w = aux(0, 4), _weights(term, 1, B, 3, np_dtype)
        xi, J = log_jlog(mul(inv(target), P[0]), np_dtype)
        return xi * w, [J * w[:, :, None]]
    if kind == PRIOR_VEC:
        target, w = aux(0, 3), _weights(term, 1, B, 3, np_dtype)
        return (P[0][:, :3] - target) * w, [_diag(w)]
    assert kind == PRIOR_XY
    target, w = aux(0, 2), _weights(term, 1, B, 2, np_dtype)
    J = np.zeros((B, 2, 3))
    J[:, :, :2] = rot(P[0])
    return (P[0][:, :2] - target) * w, [J * w[:, :, None]]


def se2_exp(xi, np_dtype):
    """(B, 3) -> (B, 4), the closed form of se2.py:239-262 with its Taylor switch"""
    eps = se2_eps(torch.float64 if np.dtype(np_dtype) == np.float64 else torch.float32)
    ux, uy, th = xi[:, 0], xi[:, 1], xi[:, 2]
    small = np.abs(th) < eps.near_zero
    th_nz = np.where(small, 1.0, th)
    sbt = np.where(small, 1 - th ** 2 / 6, np.sin(th) / th_nz)
    cm1bt = np.where(small, -th / 2 + th ** 3 / 24, (np.cos(th) - 1) / th_nz)
    return np.stack([sbt * ux + cm1bt * uy, sbt * uy - cm1bt * ux, np.cos(th), np.sin(th)], axis=1)


def retract(x, var_kind, delta, step, ignore):
    """thx_trajse2_retract on numpy arrays: x (V, B, 4), var_kind (V,), delta (B, >= 3 V), ignore (B,) | None -> (V, B, 4)"""
    out = np.empty_like(x)
    for k in range(x.shape[0]):
        d = (delta[:, 3 * k:3 * k + 3] * x.dtype.type(step)).astype(np.float64)
        xk = x[k].astype(np.float64)
        if var_kind[k]:
            new = np.concatenate([xk[:, :3] + d, np.zeros((x.shape[1], 1))], axis=1)
        else:
            new = mul(xk, se2_exp(d, x.dtype))
        out[k] = np.where(ignore[:, None] != 0, xk, new) if ignore is not None else new
    return out


class TrajSE2OracleKernels(OracleKernels):
    def __init__(self):
        super().__init__()
        self.calls = {"trajse2_eval": 0, "trajse2_error": 0, "trajse2_retract": 0}

    @staticmethod
    def _terms(table, n_terms):
        return table.numpy().view(TERM)[:n_terms]

    def trajse2_eval(self, table, n_terms, x, J, j_total, e):
        self.calls["trajse2_eval"] += 1
        B, xn = x.shape[1], x.detach().numpy()
        for term in self._terms(table, n_terms):
            err, blocks = _term(term, xn, B, xn.dtype)
            d, r0, off = err.shape[1], int(term["row0"]), int(term["j_off"])
            e[:, r0:r0 + d] = torch.from_numpy(np.ascontiguousarray(err)).to(e.dtype)
            for s, blk in enumerate(blocks):
                J[(off + 3 * d * s) * B:(off + 3 * d * (s + 1)) * B] = torch.from_numpy(np.ascontiguousarray(blk)).to(J.dtype).reshape(-1)

    def trajse2_error(self, table, n_terms, x, err):
        self.calls["trajse2_error"] += 1
        B, xn = x.shape[1], x.detach().numpy()
        acc = np.zeros(B)
        for term in self._terms(table, n_terms):
            acc += (_term(term, xn, B, xn.dtype)[0].astype(np.float64) ** 2).sum(1)
        err.copy_(torch.from_numpy(0.5 * acc).to(err.dtype))

    def trajse2_retract(self, x, var_kind, delta, step, ignore_mask, out):
        self.calls["trajse2_retract"] += 1
        new = retract(x.detach().numpy(), var_kind.numpy(), delta.detach().numpy(), step,
                      None if ignore_mask is None else ignore_mask.numpy())
        out.copy_(torch.from_numpy(new).to(out.dtype))

    def block_assemble_strided(self, asm, jacobians, errors, H, g, cache):
        self.block_assemble(asm, jacobians, errors, H, g)
