"""-m gpu: blocks of right-hand sides and the band of the inverse on the banded Cholesky factor (thx_pb_solve_multi,
thx_pb_inverse_band) and the solver surface on them.  Inputs are those of tests/test_gpu_band.py (M = L0 L0^T, random well-conditioned
band, a frame permuted by perm^-1 with garbage where nothing may be read), factorised by thx_band_factor.

Bounds.  which = 0: the solve residual ||M x - b||inf / (||M||inf ||x||inf + ||b||inf) of every vector, in the next wider format, at
most 4 x the figure of LAPACK potrs in the run's dtype on the same system + one unit roundoff (the bound of tests/test_gpu_band.py).
which = 2 / 1 are one triangular solve with the factor the device holds, so the same figure is formed with that L (L y = P b,
L^T P x = y) and bounded by 4 x LAPACK trtrs's on the same L + one unit roundoff.  The band of the inverse: max |Zb - M^-1| / max |M^-1|
over the band at most 4 x the same figure of LAPACK potrf + potri in the run's dtype + one unit roundoff."""
import numpy as np
import pytest
import torch

from tests import traj2_common
from tests.test_band_multi_host import FAMILIES, check_compute_samples, check_solver_surface
from tests.test_gpu_band import F32, F64, IDS, _K, _frame, _perm, _problem, _run, _wide

pytestmark = pytest.mark.gpu

SHAPES = [(1, 0), (5, 2), (28, 7), (64, 63), (65, 63), (130, 63), (67, 7)]
NRHS = (1, 3, 64, 65, 130)


def _dense(Lb, n, kd, w):
    L = np.zeros((n, n), dtype=w)
    for i in range(min(kd, n - 1) + 1):
        L[np.arange(i, n), np.arange(n - i)] = Lb[:n - i, i]
    return L


def _res(A, X, Bm):
    """per column of X: ||A X - B||inf / (||A||inf ||X||inf + ||B||inf)"""
    return np.abs(A @ X - Bm).max(0) / (np.abs(A).sum(1).max() * np.abs(X).max(0) + np.abs(Bm).max(0))


def _multi(Lb, n, kd, pd, rhs, which, fill=float("nan"), alias=False):
    x = rhs.clone() if alias else torch.full_like(rhs, fill)
    _K().band_solve_multi(Lb, n, kd, pd, x if alias else rhs, x, which=which)
    return x


@pytest.mark.parametrize("kind", ["identity", "reversal", "blocks"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,kd", SHAPES)
def test_multi_solve_against_lapack_and_its_own_invariants(n, kd, dtype, kind):
    perm, w, u = _perm(kind, n), _wide(dtype), torch.finfo(dtype).eps / 2
    pd = torch.from_numpy(np.ascontiguousarray(perm, dtype=np.int32)).cuda()
    worst = [0.0, 0.0, 0.0]
    for B in (1, 3):
        M64, b64 = _problem(n, kd, B)
        M = M64.to(dtype)
        Lb = _run(_frame(M, perm, dtype), n, kd, perm, b64.to(dtype).cuda(), fused=False)[0]
        Lcpu = torch.linalg.cholesky(M)
        for nrhs in NRHS:
            g = torch.Generator().manual_seed(n + nrhs)
            bb = torch.randn(B, nrhs, n, dtype=torch.float64, generator=g).to(dtype)      # banded order
            rhs = torch.empty_like(bb)
            rhs[:, :, perm] = bb                                                           # the linearization's order
            rhs = rhs.cuda()
            x0, y2 = _multi(Lb, n, kd, pd, rhs, 0), _multi(Lb, n, kd, pd, rhs, 2)
            x1 = _multi(Lb, n, kd, pd, y2, 1)
            assert torch.equal(x1, x0) and bool(torch.isfinite(x0).all())                  # 1 after 2 is 0, bitwise
            for which, src, out in ((0, rhs, x0), (2, rhs, y2), (1, y2, x0)):
                assert torch.equal(_multi(Lb, n, kd, pd, src, which, fill=0.0), out)       # whatever x held
                assert torch.equal(_multi(Lb, n, kd, pd, src, which, alias=True), out)     # x aliasing rhs
            if nrhs == 130:
                for s in (0, 64, 129):                                                     # a vector does not see its neighbours
                    assert torch.equal(_multi(Lb, n, kd, pd, rhs[:, s:s + 1].contiguous(), 0)[:, 0], x0[:, s])
            for i in range(B):
                Mi, Li = M[i].numpy().astype(w), _dense(Lb[i].cpu().numpy().astype(w), n, kd, w)
                Bi, Y, X = bb[i].numpy().astype(w).T, y2[i].cpu().numpy().astype(w).T, x0[i].cpu()[:, perm].numpy().astype(w).T
                Ld = torch.from_numpy(Li.astype(np.float64)).to(dtype)                     # (exact: its entries are dtype numbers)
                ref = (torch.cholesky_solve(bb[i].T, Lcpu[i]), torch.linalg.solve_triangular(Ld, bb[i].T, upper=False),
                       torch.linalg.solve_triangular(Ld.T, y2[i].cpu().T, upper=True))
                got = (_res(Mi, X, Bi), _res(Li, Y, Bi), _res(Li.T, X, Y))
                want = (_res(Mi, ref[0].numpy().astype(w), Bi), _res(Li, ref[1].numpy().astype(w), Bi), _res(Li.T, ref[2].numpy().astype(w), Y))
                for k in range(3):
                    assert np.isfinite(got[k]).all() and (got[k] <= 4.0 * want[k] + u).all(), (B, nrhs, i, k, got[k].max(), want[k].max())
                    worst[k] = max(worst[k], float((got[k] / np.maximum(want[k], u)).max()))
    print(f"[band_multi] solve {IDS[dtype]} n={n} kd={kd} {kind}: worst residual / max(LAPACK's, u): which=0 {worst[0]:.2f}, "
          f"which=2 {worst[1]:.2f}, which=1 {worst[2]:.2f}")


def _wide_inverse(M, w):
    X = np.linalg.inv(M.astype(np.float64)).astype(w)
    if w is np.longdouble:                                     # two Newton steps: the fp64 inverse to longdouble accuracy
        Mw, eye = M.astype(w), np.eye(M.shape[0], dtype=w)
        for _ in range(2):
            X = X + X @ (eye - Mw @ X)
    return X


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,kd", SHAPES + [(36, 11), (200, 17)])
def test_band_of_the_inverse_against_lapack(n, kd, dtype):
    perm, w, u = _perm("blocks", n), _wide(dtype), torch.finfo(dtype).eps / 2
    band = np.tril(np.ones((n, n), dtype=bool)) & ~np.tril(np.ones((n, n), dtype=bool), -kd - 1)
    for B in (1, 3):
        M64, b64 = _problem(n, kd, B)
        M = M64.to(dtype)
        Lb = _run(_frame(M, perm, dtype), n, kd, perm, b64.to(dtype).cuda(), fused=False)[0]
        Zb = torch.full_like(Lb, float("nan"))
        _K().band_inverse(Lb, n, kd, Zb)
        for j in range(max(0, n - kd), n):                     # exactly zero where j + i >= n
            assert bool((Zb[:, j, n - j:] == 0).all())
        lap = torch.cholesky_inverse(torch.linalg.cholesky(M))
        for i in range(B):
            want = _wide_inverse(M[i].numpy(), w)
            scale = np.abs(want[band]).max()
            got = float(np.abs(_dense(Zb[i].cpu().numpy().astype(w), n, kd, w) - want)[band].max() / scale)
            ref = float(np.abs(lap[i].numpy().astype(w) - want)[band].max() / scale)
            print(f"[band_multi] inverse {IDS[dtype]} n={n} kd={kd} B={B} item {i}: {got:.3e} (LAPACK potri {ref:.3e})")
            assert np.isfinite(got) and got <= 4.0 * ref + u, (got, ref)


@pytest.mark.parametrize("family,fixture", [(f, fx) for f, v in FAMILIES.items() for fx in v[0].FIXTURES])
def test_samples_and_marginals_of_the_banded_solver(family, fixture):
    import theseus_amd as th
    obj, solver, delta = check_solver_surface(th, family, fixture, None, "cuda")
    assert type(solver.K).__name__ == "HipKernels"
    if family == "traj2" and fixture == traj2_common.FIXTURES[1]:
        check_compute_samples(th, obj, solver, delta)
