"""CPU stand-in for the three banded-Cholesky wrappers of theseus_amd/kernels.py (band_factor, band_solve, band_solve_backward), on
top of the existing stand-ins: the host logic of HipBandedCholeskySolver -- band plan, buffers, the permutation contract, the fused
forward path, snapshots -- runs with ``-m "not gpu"``.  It honours what the kernels honour: only the lower triangle of the frame is
read, only the band of the permuted matrix (an entry outside it fails an assertion here, where the kernel would silently not see it),
``y`` is in banded order, everything else in the linearization's."""
import torch

from tests.oracle_kernels import OracleKernels
from tests.traj2_oracle_kernels import Traj2OracleKernels
from tests.trajse2_oracle_kernels import TrajSE2OracleKernels


def band_to_dense(Lb, n, kd):
    """(B, n, kd + 1) column-major band -> (B, n, n) lower-triangular L"""
    L = torch.zeros(Lb.shape[0], n, n, dtype=Lb.dtype, device=Lb.device)
    for i in range(min(kd, n - 1) + 1):
        L.diagonal(-i, dim1=1, dim2=2).copy_(Lb[:, :n - i, i])
    return L


def dense_to_band(L, kd, Lb):
    n = L.shape[1]
    Lb.zero_()
    for i in range(min(kd, n - 1) + 1):
        Lb[:, :n - i, i] = L.diagonal(-i, dim1=1, dim2=2)


class BandOracleMixin:
    def band_factor(self, H, n, kd, perm, damping, ellipsoidal, damping_eps, Lb, info, rhs=None, y=None):
        p = perm.long()
        assert sorted(p.tolist()) == list(range(n)) and tuple(Lb.shape) == (H.shape[0], n, kd + 1)
        Hl = torch.tril(H[:, :n, :n])
        A = Hl + torch.tril(Hl, -1).transpose(1, 2)
        if damping is not None:
            d = A.diagonal(dim1=1, dim2=2)
            add = damping.view(-1, 1) * d + damping_eps if ellipsoidal else damping.view(-1, 1).expand_as(d)
            A = A + torch.diag_embed(add)
        Ap = A[:, p][:, :, p]
        idx = torch.arange(n)
        outside = (idx[:, None] - idx[None, :]).abs() > kd
        assert not (Ap[:, outside] != 0).any(), "the permuted matrix has entries outside the band the kernel reads"
        Lc, inf = torch.linalg.cholesky_ex(Ap)
        dense_to_band(Lc, kd, Lb)
        info.copy_(inf.to(info.dtype))
        if rhs is not None:
            y.copy_(torch.linalg.solve_triangular(Lc, rhs[:, p].unsqueeze(2), upper=False).squeeze(2))

    def band_solve(self, Lb, n, kd, perm, rhs, x):
        p = perm.long()
        x[:, p] = torch.cholesky_solve(rhs[:, p].unsqueeze(2), band_to_dense(Lb, n, kd)).squeeze(2)

    def band_solve_backward(self, Lb, n, kd, perm, y, x):
        L = band_to_dense(Lb, n, kd)
        x[:, perm.long()] = torch.linalg.solve_triangular(L.transpose(1, 2), y.clone().unsqueeze(2), upper=True).squeeze(2)


class BandOracleKernels(BandOracleMixin, OracleKernels):
    pass


class BandTraj2OracleKernels(BandOracleMixin, Traj2OracleKernels):
    pass


class BandTrajSE2OracleKernels(BandOracleMixin, TrajSE2OracleKernels):
    pass
