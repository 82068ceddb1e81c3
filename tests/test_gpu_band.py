"""-m gpu: the banded Cholesky solver (thx_band_factor / thx_band_solve*, HipBandedCholeskySolver) against CPU LAPACK in the same
dtype.

  * factor and solve residuals, measured in the next wider format, at most 4 x LAPACK's (potrf + potrs) + one unit roundoff -- the
    bound of tests/test_gpu_lu.py -- on M = L0 L0^T with L0 a random lower band (well conditioned, bandwidth exactly kd), presented
    in a frame permuted by perm^-1 whose upper triangle and padding hold values that would wreck the result if read;
  * the three solve entry points agree bitwise where they overlap;
  * every damping mode against LAPACK on the damped matrix, H unchanged;
  * one indefinite item: info in the banded order, the other items keep their bits, the solver raises, the LM ends with FAIL;
  * independence from what the output buffers held, aliasing, run-to-run reproducibility;
  * the trajectory fixtures end to end with HipBandedCholeskySolver at the tolerances of the dense solver's tests; the fp32 solve
    residual on a larger random planner; an SE3 odometry chain (the block-compact path).

Shapes (n, kd) cross every boundary of the design: kd = 0, kd = n - 1, the limit kd = 63 at n = 64 (one window, no refill), 65 and
130 (the fused forward substitution's second and third row per lane), n no multiple of the 8-column chunk, kd odd and even (the
folded update rectangle pairs the middle row with itself for odd kd), more update elements than lanes (kd >= 11), the planner's
N = 100 shape (404, 7); batches 1, 3, 65 (no multiple of the four problems per workgroup) and 257."""
import functools

import numpy as np
import pytest
import torch

from tests import traj2_common, trajse2_common
from tests.helpers import load_golden
from tests.test_band_host import _lm

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
IDS = {F32: "f32", F64: "f64"}
SHAPES = [(1, 0), (5, 0), (5, 2), (4, 3), (28, 7), (36, 11), (64, 63), (65, 63), (130, 63), (67, 7), (200, 17), (404, 7)]
GARBAGE = 7.0e7   # what the frame holds where the kernel must not read


def _K():
    from theseus_amd.kernels import default_kernels
    return default_kernels()


def _ld(n):
    return (n + 31) // 32 * 32


def _batches(n, kd):
    return (1, 3, 65, 257) if (n, kd) == (67, 7) else (1, 3, 65)


@functools.lru_cache(maxsize=None)
def _problem(n, kd, B):
    """(M (B, n, n), b (B, n)) in fp64 on the CPU: M = L0 L0^T, diag(L0) in [1, 2], the kd sub-diagonals uniform in
    +-0.5 / sqrt(kd + 1).  Made once per shape and shared; nobody writes to them."""
    g = torch.Generator().manual_seed(1000 * n + 10 * kd + B)
    L0 = torch.zeros(B, n, n, dtype=F64)
    for i in range(min(kd, n - 1) + 1):
        d = L0.diagonal(-i, dim1=1, dim2=2)
        r = torch.rand(B, n - i, dtype=F64, generator=g)
        d.copy_(1 + r if i == 0 else (r - 0.5) / np.sqrt(kd + 1))
    return L0 @ L0.transpose(1, 2), torch.randn(B, n, dtype=F64, generator=g)


def _perm(kind, n):
    if kind == "identity":
        return np.arange(n)
    if kind == "reversal":
        return np.arange(n)[::-1].copy()
    blocks = [np.arange(s, min(s + 2, n)) for s in range(0, n, 2)]   # variables of two columns (the last may have one)
    order = np.random.default_rng(n).permutation(len(blocks))
    return np.concatenate([blocks[k] for k in order])


def _frame(M, perm, dtype):
    """The (B, ld, ld) frame in the LINEARIZATION's order: H[perm[i], perm[j]] = M[i, j] in the lower triangle, GARBAGE elsewhere."""
    B, n = M.shape[0], M.shape[1]
    inv = np.argsort(perm)
    H = torch.full((B, _ld(n), _ld(n)), GARBAGE, dtype=dtype)
    low = torch.tril(torch.ones(n, n, dtype=torch.bool))
    H[:, :n, :n] = torch.where(low, M[:, inv][:, :, inv].to(dtype), torch.tensor(GARBAGE, dtype=dtype))
    return H.cuda()


def _run(H, n, kd, perm, rhs, lam=None, ell=False, eps=1e-8, fill=None, fused=True):
    """fused: thx_band_factor with rhs + thx_band_solve_backward; else thx_band_factor + thx_band_solve.  Fresh buffers holding
    ``fill`` (None: torch.empty).  -> (Lb, info, y | None, x)"""
    K, B, dt = _K(), H.shape[0], H.dtype
    mk = (lambda *s, dtype=dt: torch.empty(*s, dtype=dtype, device="cuda")) if fill is None else \
        (lambda *s, dtype=dt: torch.full(s, fill if dtype != torch.int32 else 0x7FC00000, dtype=dtype, device="cuda"))
    pd = torch.from_numpy(np.ascontiguousarray(perm, dtype=np.int32)).cuda()
    Lb, info, x = mk(B, n, kd + 1), mk(B, dtype=torch.int32), mk(B, n)
    y = None
    if fused:
        y = mk(B, n)
        K.band_factor(H, n, kd, pd, lam, ell, eps, Lb, info, rhs=rhs, y=y)
        K.band_solve_backward(Lb, n, kd, pd, y, x)
    else:
        K.band_factor(H, n, kd, pd, lam, ell, eps, Lb, info)
        K.band_solve(Lb, n, kd, pd, rhs, x)
    torch.cuda.synchronize()
    return Lb, info, y, x


def _wide(dtype):
    return np.float64 if dtype == F32 else np.longdouble


def _band_of(L, kd):
    """(n, n) lower triangular -> (n, kd + 1) band by columns (zeros past the end)"""
    n = L.shape[0]
    Lb = np.zeros((n, kd + 1), dtype=L.dtype)
    for i in range(min(kd, n - 1) + 1):
        Lb[:n - i, i] = np.diagonal(L, -i)
    return Lb


def _figures(M, Lb, x, b, kd, dtype):
    """(||L L^T - M||_max / ||M||_max,  ||M x - b||_inf / (||M||_inf ||x||_inf + ||b||_inf)) in the next wider format; L given as
    its band: (L L^T)(j + c, j + a) += L(j + c, j) L(j + a, j), diagonal by diagonal (both matrices vanish outside the band)."""
    w = _wide(dtype)
    M, Lb, x, b = (np.asarray(a).astype(w) for a in (M, Lb, x, b))
    n = M.shape[0]
    fac = w(0)
    for off in range(min(kd, n - 1) + 1):
        acc = np.zeros(n - off, dtype=w)                      # (L L^T)(r + off, r), r = 0 .. n - off - 1
        for a in range(kd + 1 - off):                         # column j = r - a contributes L(j + a + off, j) L(j + a, j)
            m = n - off - a
            if m <= 0:
                break
            acc[a:] += Lb[:m, a + off] * Lb[:m, a]
        fac = max(fac, np.abs(acc - np.diagonal(M, -off)).max())
    res = np.abs(M @ x - b).max() / (np.abs(M).sum(1).max() * np.abs(x).max() + np.abs(b).max())
    return float(fac / np.abs(M).max()), float(res)


def _lapack_figures(Md, b, kd, dtype):
    """The same two figures for CPU LAPACK's potrf + potrs of the same matrix in the same dtype."""
    L = torch.linalg.cholesky(Md)
    x = torch.cholesky_solve(b.unsqueeze(1), L).squeeze(1)
    return _figures(Md.numpy(), _band_of(L.numpy(), kd), x.numpy(), b.numpy(), kd, dtype)


def _check_against_lapack(Md, b, perm, Lb, x, kd, dtype, what):
    """Md (B, n, n), b (B, n): the (damped) matrices in the BANDED order and the right-hand sides in the linearization's, on the CPU
    in ``dtype``; x in the linearization's order.  Items 0 .. 3 -- the four waves of the first workgroup, each with its own LDS
    window -- and B / 2 + 1, B - 2, B - 1, which sit on other waves of later workgroups."""
    u = torch.finfo(dtype).eps / 2
    B, n = Md.shape[0], Md.shape[1]
    Lb, x = Lb.cpu(), x.cpu()
    for i in sorted({k for k in (0, 1, 2, 3, B // 2 + 1, B - 2, B - 1) if 0 <= k < B}):
        bp = b[i][perm]
        hip = _figures(Md[i].numpy(), Lb[i].numpy(), x[i][perm].numpy(), bp.numpy(), kd, dtype)
        ref = _lapack_figures(Md[i], bp, kd, dtype)
        print(f"[band] {what} {IDS[dtype]} n={n} kd={kd} B={B} item {i}: factor {hip[0]:.3e} (LAPACK {ref[0]:.3e}), "
              f"solve {hip[1]:.3e} (LAPACK {ref[1]:.3e})")
        assert all(np.isfinite(ref)) and all(np.isfinite(hip))
        if n >= 4:   # (a 1 x 1 system can come out exact; so can the factor of a diagonal one, a square root per entry)
            assert (ref[0] > 0 or kd == 0) and ref[1] > 0
        for k in (0, 1):
            assert hip[k] <= 4.0 * ref[k] + u, (what, i, k, hip, ref)


def _damped(M, lam, ell, eps):
    """M + D evaluated in M's dtype with the kernel's expression (x + (lam x + eps) / x + lam on the diagonal)."""
    Md = M.clone()
    if lam is not None:
        d = torch.diagonal(Md, dim1=1, dim2=2)
        lamc = lam.view(-1, 1)
        d.copy_(d + (lamc * d + eps) if ell else d + lamc)
    return Md


# ---- 1. against LAPACK -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["identity", "reversal", "blocks"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,kd", SHAPES)
def test_factor_and_solves_against_lapack(n, kd, dtype, kind):
    perm = _perm(kind, n)
    for B in _batches(n, kd):
        M64, b64 = _problem(n, kd, B)
        M, b = M64.to(dtype), b64.to(dtype)
        H, rhs = _frame(M, perm, dtype), b.cuda()
        Lb, info, y, x = _run(H, n, kd, perm, rhs, fused=True)
        assert info.cpu().tolist() == [0] * B
        for j in range(max(0, n - kd), n):            # zeros where j + i >= n
            assert bool((Lb[:, j, n - j:] == 0).all())
        Lb2, info2, _, x2 = _run(H, n, kd, perm, rhs, fused=False)
        assert torch.equal(Lb, Lb2) and torch.equal(info, info2) and torch.equal(x, x2)   # bitwise
        _check_against_lapack(M, b, perm, Lb, x, kd, dtype, kind)


# ---- 2. damping ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["none", "scalar", "per_item", "ellipsoidal"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_damping_modes_against_lapack_on_the_damped_matrix(dtype, mode):
    n, kd, B = 36, 11, 3
    perm = _perm("blocks", n)
    M64, b64 = _problem(n, kd, B)
    M, b = M64.to(dtype), b64.to(dtype)
    H = _frame(M, perm, dtype)
    before = H.clone()
    lam = {"none": None, "scalar": torch.full((B,), 0.37, dtype=dtype), "per_item": torch.tensor([0.0, 0.5, 3.0], dtype=dtype),
           "ellipsoidal": torch.tensor([0.01, 0.5, 2.0], dtype=dtype)}[mode]
    ell, eps = mode == "ellipsoidal", 1e-3 if mode == "ellipsoidal" else 1e-8
    Lb, info, _, x = _run(H, n, kd, perm, b.cuda(), lam=lam.cuda() if lam is not None else None, ell=ell, eps=eps)
    assert torch.equal(H, before) and info.cpu().tolist() == [0] * B
    _check_against_lapack(_damped(M, lam, ell, eps), b, perm, Lb, x, kd, dtype, mode)
    if mode != "none":   # (the damping really went in)
        plain = _run(H, n, kd, perm, b.cuda())[0]
        assert not torch.equal(plain[1], Lb[1])


# ---- 3. one indefinite item ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_an_indefinite_item_is_reported_in_the_banded_order_and_the_others_keep_their_bits(dtype):
    n, kd, B = 36, 11, 3
    perm = _perm("blocks", n)
    M64, b64 = _problem(n, kd, B)
    H, rhs = _frame(M64.to(dtype), perm, dtype), b64.to(dtype).cuda()
    good = _run(H, n, kd, perm, rhs, fill=0.0)
    k = int(perm[3])
    H[1, k, k] = -H[1, k, k]          # banded column 3 of item 1
    Mbad = M64.to(dtype).clone()
    Mbad[1, 3, 3] = -Mbad[1, 3, 3]
    assert torch.linalg.cholesky_ex(Mbad).info.tolist() == [0, 4, 0]      # (the premise, by LAPACK alone)
    Lb, info, y, x = _run(H, n, kd, perm, rhs, fill=0.0)
    assert info.cpu().tolist() == [0, 4, 0]
    for a, c in zip((Lb, y, x), (good[0], good[2], good[3])):
        assert torch.equal(a[[0, 2]], c[[0, 2]])


def _se3_chain(th, B=3, P=8, weight=1.0, seed=0):
    """An SE3 odometry chain: Between (i, i + 1) and (i, i + 2), one prior on pose 0 -- block half-bandwidth 2, kd = 17."""
    from tests.test_gpu_lm import build_objective
    g = torch.Generator().manual_seed(seed)

    def poses(*shape):
        xi = 0.3 * torch.randn(*shape, 6, dtype=F64, generator=g)
        W = torch.zeros(*shape, 3, 3, dtype=F64)
        W[..., 0, 1], W[..., 0, 2], W[..., 1, 2] = -xi[..., 5], xi[..., 4], -xi[..., 3]
        R = torch.linalg.matrix_exp(W - W.transpose(-1, -2))
        return torch.cat([R, xi[..., :3].unsqueeze(-1)], dim=-1).numpy()
    edges = np.array([(i, i + 1) for i in range(P - 1)] + [(i, i + 2) for i in range(P - 2)])
    E = edges.shape[0]
    spec = dict(P=P, poses0=poses(B, P), edges=edges, meas=poses(B, E), prior_idx=np.array([0]), prior_target=poses(B, 1),
                w_between=weight * (1 + torch.rand(B, E, 6, dtype=F64, generator=g)).numpy(),
                w_prior=weight * np.ones((B, 1, 6)))
    return build_objective(th, spec)


def test_one_indefinite_item_raises_from_the_solver_and_fails_the_loop(monkeypatch):
    """The traj2 fixture, batch 3: after every linearization the diagonal entry at BANDED column 3 of item 1 changes sign (the
    assembly itself is untouched: the frame is edited behind it).  solve() raises for item 1 alone with the minor counted in the
    banded order, info is [0, 4, 0], and the LM loop ends with FAIL status."""
    import warnings
    import theseus_amd as th
    obj, _, _ = traj2_common.build(th, load_golden(traj2_common.FIXTURES[1]), device="cuda")
    opt = th.LevenbergMarquardt(obj, linear_solver_cls=th.HipBandedCholeskySolver, **traj2_common.LM_KW)
    solver, lin = opt.linear_solver, opt.linear_solver.linearization
    obj.update()
    lin.linearize()
    with torch.no_grad():
        good = solver.solve(damping=traj2_common.LM_DAMPING).clone()
    k = int(solver.band_plan().perm[3])
    assemble = type(lin)._assemble

    def flipped(self):
        assemble(self)
        self.H[1, k, k] = -self.H[1, k, k]
    monkeypatch.setattr(type(lin), "_assemble", flipped)
    lin.linearize()
    with torch.no_grad():
        with pytest.raises(RuntimeError, match=r"linalg\.cholesky: \(Batch element 1\).*leading minor of order 4 is not positive-definite"):
            solver.solve(damping=traj2_common.LM_DAMPING)
        assert solver.info.cpu().tolist() == [0, 4, 0]
        delta = solver.solve(damping=traj2_common.LM_DAMPING, check_info=False)
    assert torch.equal(delta[[0, 2]], good[[0, 2]])      # the other items keep their bits through the solver as well
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        with torch.no_grad():
            info = opt.optimize(damping=traj2_common.LM_DAMPING)
    assert all(s == th.NonlinearOptimizerStatus.FAIL for s in info.status)


def test_a_failed_item_raises_from_the_solver_and_fails_the_loop():
    """All weights zero: AtA = 0, the first pivot is not positive.  HipBandedCholeskySolver.solve() raises the Cholesky solvers'
    error (its minor counted in the banded order), the LM loop ends with FAIL status: a reported failure, not a fault."""
    import warnings
    import theseus_amd as th
    obj, _ = _se3_chain(th, weight=0.0)
    opt = th.LevenbergMarquardt(obj, linear_solver_cls=th.HipBandedCholeskySolver, max_iterations=3)
    obj.update()
    opt.linear_solver.linearization.linearize()
    with pytest.raises(RuntimeError, match=r"linalg\.cholesky: \(Batch element 0\).*leading minor of order 1 is not positive-definite"):
        opt.linear_solver.solve(damping=None)
    assert opt.linear_solver.info.cpu().tolist() == [1, 1, 1]
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        info = opt.optimize(damping=0.0, ellipsoidal_damping=False)
    assert all(s == th.NonlinearOptimizerStatus.FAIL for s in info.status)


# ---- 4. stale buffers, aliasing, reproducibility ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kd,B,dtype", [(36, 11, 3, F32), (130, 63, 3, F64), (67, 7, 65, F32)])
def test_results_do_not_depend_on_what_the_buffers_held(n, kd, B, dtype):
    perm = _perm("blocks", n)
    M64, b64 = _problem(n, kd, B)
    H, rhs = _frame(M64.to(dtype), perm, dtype), b64.to(dtype).cuda()
    lam = torch.full((B,), 0.1, dtype=dtype, device="cuda")
    base = _run(H, n, kd, perm, rhs, lam=lam, ell=True, fill=0.0)
    for fill in (float("nan"), -3.0e30, None):       # NaN, garbage, whatever the allocator hands out (a second run)
        again = _run(H, n, kd, perm, rhs, lam=lam, ell=True, fill=fill)
        for a, c in zip(base, again):
            assert torch.equal(a, c)
    unfused = _run(H, n, kd, perm, rhs, lam=lam, ell=True, fill=float("nan"), fused=False)
    assert torch.equal(unfused[0], base[0]) and torch.equal(unfused[3], base[3])
    # output aliasing input in the two solves
    K = _K()
    pd = torch.from_numpy(np.ascontiguousarray(perm, dtype=np.int32)).cuda()
    x = rhs.clone()
    K.band_solve(base[0], n, kd, pd, x, x)
    yx = base[2].clone()
    K.band_solve_backward(base[0], n, kd, pd, yx, yx)
    torch.cuda.synchronize()
    assert torch.equal(x, base[3]) and torch.equal(yx, base[3])


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,fixture", [("traj2", f) for f in traj2_common.FIXTURES] + [("trajse2", f) for f in trajse2_common.FIXTURES])
def test_banded_lm_reproduces_the_reference_iterates_and_implicit_gradients(family, fixture):
    import theseus_amd as th
    if family == "traj2":
        from tests.test_traj2_host import check_implicit_gradients, check_iterates
        common, packed, kd_max = traj2_common, "PackedTrajectory2D", 7
    else:
        from tests.test_push2_host import check_implicit_gradients, check_iterates
        common, packed, kd_max = trajse2_common, "PackedTrajectorySE2", 11
    g = load_golden(fixture)
    with torch.no_grad():
        _, opt, _, _, info = _lm(th, common, g, None, device="cuda", track_err_history=True, track_state_history=True)
    assert type(opt.linear_solver) is th.HipBandedCholeskySolver and opt.linear_solver.band_plan().kd <= kd_max
    assert type(opt.linear_solver.linearization.packed).__name__ == packed      # still the fused family
    check_iterates(g, info, g["var_order"].tolist())
    _, opt, leaves, sol, _ = _lm(th, common, g, None, device="cuda", backward_mode="implicit")
    assert type(opt.linear_solver.linearization.packed).__name__ == packed
    check_implicit_gradients(g, leaves, sol, g["var_order"].tolist())


def test_unrolled_gradients_equal_the_dense_solvers():
    """backward_mode="unroll": factor_snapshot / solve_with_snapshot.  Two evaluations of the same maths: 1e-9 of the largest entry
    (tests/test_traj2_host.py)."""
    import theseus_amd as th
    from tests.test_traj2_host import _lm as dense_lm
    g = load_golden(traj2_common.FIXTURES[1])
    names = g["var_order"].tolist()
    grads = {}
    for name in ("banded", "dense"):
        if name == "banded":
            _, opt, leaves, sol, _ = _lm(th, traj2_common, g, None, device="cuda", backward_mode="unroll")
        else:
            _, opt, leaves, sol, _ = dense_lm(th, g, None, device="cuda", backward_mode="unroll")
        assert type(opt.linear_solver).__name__ == {"banded": "HipBandedCholeskySolver", "dense": "HipCholeskySolver"}[name]
        (traj2_common.state_of(sol, names) ** 2).sum().backward()
        grads[name] = {k: v.grad.cpu().numpy() for k, v in leaves.items()}
    for k, want in grads["dense"].items():
        assert np.abs(want).max() > 0
        np.testing.assert_allclose(grads["banded"][k], want, rtol=0, atol=1e-9 * np.abs(want).max(), err_msg=k)


def test_fp32_solve_residual_on_a_random_planner_is_the_dense_solvers():
    """random_problem(B = 70, N = 40): n = 164.  After 5 LM iterations the last linearization is solved by both solvers; the banded
    delta's residual (formed in fp64) is at most 4 x the dense solver's + one unit roundoff, item by item."""
    import theseus_amd as th
    obj, _, _ = traj2_common.build(th, traj2_common.random_problem(70, 40, 5), device="cuda", dtype=F32, N=40)
    opt = th.LevenbergMarquardt(obj, **traj2_common.LM_KW)
    with torch.no_grad():
        opt.optimize(damping=traj2_common.LM_DAMPING)
        dense = opt.linear_solver
        lin = dense.linearization
        lin.linearize()
        banded = th.HipBandedCholeskySolver(obj)
        banded.linearization = lin                      # the SAME linearization for both
        assert type(lin.packed).__name__ == "PackedTrajectory2D" and lin.n == 164
        lam = traj2_common.LM_DAMPING
        d_dense = dense.solve(damping=lam).double().cpu()
        d_band = banded.solve(damping=lam).double().cpu()
        assert banded.band_plan().kd <= 7
        A = lin.AtA.double().cpu()
        A = A + torch.diag_embed(lam * A.diagonal(dim1=1, dim2=2) + 1e-8)
        gvec = lin.g.double().cpu()
    u = torch.finfo(F32).eps / 2

    def res(d):
        r = ((A @ d.unsqueeze(2)).squeeze(2) - gvec).abs().amax(1)
        return r / (A.abs().sum(2).amax(1) * d.abs().amax(1) + gvec.abs().amax(1))
    rb, rd = res(d_band), res(d_dense)
    print(f"[band] fp32 planner n=164 B=70: residual banded max {rb.max():.3e}, dense max {rd.max():.3e}")
    assert bool(torch.isfinite(rb).all()) and bool((rb <= 4.0 * rd + u).all()), (rb.max(), rd.max())


def test_se3_odometry_chain_takes_the_block_compact_path():
    """8 poses, Between (i, i + 1) and (i, i + 2), one prior, batch 3, fp64: one LM step equals HipCholeskySolver's to 1e-10."""
    import theseus_amd as th
    out = {}
    for name, cls in (("banded", th.HipBandedCholeskySolver), ("dense", th.HipCholeskySolver)):
        obj, poses = _se3_chain(th)
        opt = th.LevenbergMarquardt(obj, linear_solver_cls=cls, max_iterations=1, step_size=1.0)
        with torch.no_grad():
            opt.optimize(damping=0.1)
        assert opt.linear_solver.linearization._compact and opt.linear_solver.linearization.n == 48
        if name == "banded":
            assert opt.linear_solver.band_plan().kd == 17 and opt.linear_solver._frame is not None
        out[name] = torch.stack([p.tensor for p in poses]).cpu()
    start = torch.stack([p.tensor for p in _se3_chain(th)[1]]).cpu()
    assert float((out["dense"] - start).abs().max()) > 1e-2      # (the step is not a trivial one)
    assert float((out["banded"] - out["dense"]).abs().max()) <= 1e-10 * float(out["dense"].abs().max())
