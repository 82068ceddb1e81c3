"""CPU stand-ins for the two multi-vector wrappers on the band factor (theseus_amd/kernels.py: band_solve_multi, band_inverse) on
top of tests/band_oracle_kernels.py, so the solver surface built on them runs with ``-m "not gpu"``.  Same contracts: which = 0 in
and out in the linearization's order, 2 out in banded order, 1 in banded order; Zb is the band of (L L^T)^-1 in banded order."""
import torch

from tests.band_oracle_kernels import BandOracleMixin, band_to_dense, dense_to_band
from tests.oracle_kernels import OracleKernels
from tests.traj2_oracle_kernels import Traj2OracleKernels
from tests.trajse2_oracle_kernels import TrajSE2OracleKernels


class BandMultiOracleMixin(BandOracleMixin):
    def band_solve_multi(self, Lb, n, kd, perm, rhs, x, which=0):
        p = perm.long()
        L = band_to_dense(Lb, n, kd)
        v = rhs.transpose(1, 2).clone()                                   # (B, n, k)
        if which != 1:
            v = torch.linalg.solve_triangular(L, v[:, p], upper=False)
        if which != 2:
            v = torch.linalg.solve_triangular(L.transpose(1, 2), v, upper=True)
            out = torch.empty_like(v)
            out[:, p] = v
            v = out
        x.copy_(v.transpose(1, 2))

    def chol_solve_multi(self, L, n, panels, rhs, x, which=0):
        """(the dense solver's counterpart, for the comparison of the two solvers' covariances)"""
        Ln, v = torch.tril(L[:, :n, :n]), rhs.transpose(1, 2).clone()
        if which != 1:
            v = torch.linalg.solve_triangular(Ln, v, upper=False)
        if which != 2:
            v = torch.linalg.solve_triangular(Ln.transpose(1, 2), v, upper=True)
        x.copy_(v.transpose(1, 2))

    def band_inverse(self, Lb, n, kd, Zb):
        L = band_to_dense(Lb, n, kd)
        dense_to_band(torch.tril(torch.cholesky_inverse(L)), kd, Zb)


class BandMultiOracleKernels(BandMultiOracleMixin, OracleKernels):
    pass


class BandMultiTraj2OracleKernels(BandMultiOracleMixin, Traj2OracleKernels):
    pass


class BandMultiTrajSE2OracleKernels(BandMultiOracleMixin, TrajSE2OracleKernels):
    pass
