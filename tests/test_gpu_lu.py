"""-m gpu: the pivoted LU solver (thx_lu_factor / thx_lu_solve*, HipLUSolver) against CPU LAPACK in the same dtype.

  * the pivot sequence on matrices whose partial pivoting is forced (LAPACK itself is asserted to return the planted permutation);
  * factor and solve residuals, measured in the next wider format, at most 4 x LAPACK's + one unit roundoff;
  * symmetric indefinite systems with a zero diagonal: the Cholesky reports a failure, the LU solves them;
  * an exactly singular item: info as LAPACK's, the other items keep their bits, HipLUSolver raises, the LM ends with FAIL;
  * independence from what the output buffers held;
  * the fixtures of the Cholesky solver's end-to-end tests, with HipLUSolver, at the same tolerances.

Sizes cross every boundary of the 32-wide panel and of the 128 x 64 trailing tile; batches of 1, 3 and 65 problems."""
import numpy as np
import pytest
import torch

from tests.helpers import golden_problem, load_golden

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
IDS = {F32: "f32", F64: "f64"}


def _K():
    from theseus_amd.kernels import default_kernels
    return default_kernels()


def _ld(n):
    return (n + 31) // 32 * 32


def _lu(M, lam=None, ell=False, eps=1e-8, rhs=None, fill=None):
    """General mode: thx_lu_factor (+ thx_lu_solve_forward / _backward with ``rhs``) of full (B, n, n) matrices."""
    return _lu_n(_K(), M, M.shape[1], lam, ell, eps, False, rhs, fill)


def _lu_n(K, M, n, lam, ell, eps, symmetric_lower, rhs, fill):
    """... into fresh buffers holding ``fill`` (None: torch.empty); symmetric_lower: M is a (B, ld, ld) frame."""
    B = M.shape[0]
    ld = M.shape[-1] if symmetric_lower else _ld(n)
    mk = (lambda *s, dt=M.dtype: torch.empty(*s, dtype=dt, device="cuda")) if fill is None else \
        (lambda *s, dt=M.dtype: torch.full(s, fill, dtype=dt, device="cuda") if dt != torch.int32
         else torch.full(s, 0x7FC00000 if fill != 0 else 0, dtype=dt, device="cuda"))
    LU, piv, info = mk(B, ld, ld), mk(B, n, dt=torch.int32), mk(B, dt=torch.int32)
    K.lu_factor(M, n, lam, ell, eps, LU, piv, info, symmetric_lower=symmetric_lower)
    x = y = None
    if rhs is not None:
        y, x = mk(B, n), mk(B, n)
        K.lu_solve_forward(LU, n, piv, rhs, y)
        K.lu_solve_backward(LU, n, y, x)
    torch.cuda.synchronize()
    return LU, piv, info, y, x


def _wide(dtype):
    return np.float64 if dtype == F32 else np.longdouble


def _permuted(M, piv0):
    """P M for 0-based getrf pivots (numpy, any dtype)."""
    A = M.copy()
    for k, p in enumerate(piv0):
        if p != k:
            A[[k, p]] = A[[p, k]]
    return A


def _figures(M, LU, piv0, x, b, dtype):
    """(||P M - L U||_max / ||M||_max,  ||M x - b||_inf / (||M||_inf ||x||_inf + ||b||_inf)) in the next wider format."""
    w = _wide(dtype)
    M, LU, x, b = (np.asarray(a).astype(w) for a in (M, LU, x, b))
    n = M.shape[0]
    L = np.tril(LU, -1) + np.eye(n, dtype=w)
    U = np.triu(LU)
    fac = np.abs(_permuted(M, piv0) - L @ U).max() / np.abs(M).max()
    res = np.abs(M @ x - b).max() / (np.abs(M).sum(1).max() * np.abs(x).max() + np.abs(b).max())
    return float(fac), float(res)


def _lapack_figures(Md, b, dtype):
    """The same two figures for CPU LAPACK's factor and solve of the same matrix in the same dtype."""
    Mc, bc = Md.cpu(), b.cpu()
    LUr, pr = torch.linalg.lu_factor(Mc)
    xr = torch.linalg.lu_solve(LUr, pr, bc.unsqueeze(-1)).squeeze(-1)
    return _figures(Mc.numpy(), LUr.numpy(), (pr.numpy() - 1).tolist(), xr.numpy(), bc.numpy(), dtype)


def _check_against_lapack(Md, LU, piv, x, b, dtype, items, what):
    """Md: the (damped) matrices as the factorisation sees them, in ``dtype``.  Returns the worst ratios."""
    u = torch.finfo(dtype).eps / 2
    n = Md.shape[1]
    worst = [0.0, 0.0]
    for i in items:
        hip = _figures(Md[i].cpu().numpy(), LU[i, :n, :n].cpu().numpy(), piv[i].cpu().tolist(), x[i].cpu().numpy(), b[i].cpu().numpy(),
                       dtype)
        ref = _lapack_figures(Md[i], b[i], dtype)
        print(f"[lu] {what} {IDS[dtype]} n={n} item {i}: factor {hip[0]:.3e} (LAPACK {ref[0]:.3e}), solve {hip[1]:.3e} "
              f"(LAPACK {ref[1]:.3e})")
        for k in (0, 1):
            assert hip[k] <= 4.0 * ref[k] + u, (what, i, k, hip, ref)
            worst[k] = max(worst[k], hip[k] / max(ref[k], 1e-300))
    return worst


def _damped(M, lam, ell, eps):
    """M + D evaluated in M's dtype with the kernel's expression (x + (lam x + eps) / x + lam on the diagonal)."""
    if lam is None:
        return M.clone()
    Md = M.clone()
    d = torch.diagonal(Md, dim1=1, dim2=2)
    lamc = lam.view(-1, 1)
    d.copy_(d + (lamc * d + eps) if ell else d + lamc)
    return Md


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


# ---- 1. the pivot sequence --------------------------------------------------------------------------------------------------------
def _planted(B, n, dtype, seed):
    """M = P^T L U: unit-lower L with |l| <= 0.5, U with |u_kk| in [1, 2] (random sign) and |u_kj| <= 1 -- at every step the true
    pivot is at least twice every competitor, so partial pivoting has to recover P.

    The strictly-lower entries of L are drawn from [-0.5, 0.5] * min(1, 32 / n).  With the full range at every n the premise does
    not survive rounding: the error of the computed Schur complements grows with L^-1, and CPU LAPACK itself loses the planted
    permutation at n = 200 in fp32 (six seeds of six) and at n = 384 in fp64 (likewise), once in six at n = 129 in fp32.  With this
    range LAPACK recovers it for every size and dtype used below (eight seeds of eight each), and the test asserts that first."""
    g = _gen(seed)
    r = lambda *s: torch.rand(*s, dtype=F64, device="cuda", generator=g)  # noqa: E731
    L = torch.tril((r(B, n, n) - 0.5) * min(1.0, 32.0 / n), -1) + torch.eye(n, dtype=F64, device="cuda")
    U = torch.triu(2.0 * r(B, n, n) - 1.0, 1) + torch.diag_embed((1.0 + r(B, n)) * torch.sign(r(B, n) - 0.5))
    perm = torch.stack([torch.randperm(n, device="cuda", generator=g) for _ in range(B)])
    LUm = L @ U
    M = torch.empty_like(LUm)
    # row perm[b, k] of M is row k of L U:  (P M)[k] = M[perm[k]]
    M.scatter_(1, perm.view(B, n, 1).expand(B, n, n), LUm)
    return M.to(dtype), perm


def _perm_of_pivots(piv0, n):
    rows = list(range(n))
    for k, p in enumerate(piv0):
        rows[k], rows[p] = rows[p], rows[k]
    return rows


@pytest.mark.parametrize("n,B,dtype", [(5, 1, F32), (32, 3, F64), (33, 3, F32), (127, 65, F32), (128, 3, F64), (129, 3, F64),
                                       (200, 3, F32), (384, 1, F64)])
def test_pivot_sequence_is_lapacks(n, B, dtype):
    M, perm = _planted(B, n, dtype, seed=1000 + n)
    _, pr = torch.linalg.lu_factor(M.cpu())
    pr = (pr - 1).tolist()
    for b in range(B):   # the premise, by the reference alone: LAPACK recovers the planted permutation
        assert _perm_of_pivots(pr[b], n) == perm[b].tolist(), b
    Mc = M.clone()
    LU, piv, info, _, _ = _lu(M)
    assert piv.cpu().tolist() == pr
    assert info.cpu().tolist() == [0] * B
    assert torch.equal(M, Mc)


# ---- 2. factor and solve quality ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,B,dtype", [(5, 3, F64), (32, 3, F32), (127, 3, F64), (128, 65, F32), (200, 3, F64), (384, 3, F32)])
def test_general_matrices_vs_lapack(n, B, dtype):
    g = _gen(n + B)
    M = torch.randn(B, n, n, dtype=F64, device="cuda", generator=g).to(dtype)
    b = torch.randn(B, n, dtype=F64, device="cuda", generator=g).to(dtype)
    LU, piv, info, _, x = _lu(M, rhs=b)
    assert info.cpu().tolist() == [0] * B
    _check_against_lapack(M, LU, piv, x, b, dtype, sorted({0, B // 2, B - 1}), "general")


SPD_CASES = [(33, 3, F64, "scalar"), (129, 65, F32, "ellipsoidal"), (200, 3, F32, None), (127, 3, F64, "ellipsoidal"),
             (384, 3, F32, "scalar")]


@pytest.mark.parametrize("n,B,dtype,damping", SPD_CASES)
def test_symmetric_lower_frames_vs_lapack_and_cholesky(n, B, dtype, damping):
    """Symmetric-lower mode on the frame the assemble kernels write (NaN above the diagonal: never read), scalar / ellipsoidal
    damping with one lambda per problem; x also against the Cholesky's at the tolerances of test_right_looking_modes_vs_lapack."""
    from tests.test_gpu_chol_schedules import _spd
    from tests.gpu_helpers import factor_and_solve
    M = _spd(B, n, dtype, seed=3 * n + B)
    ld = _ld(n)
    H = torch.zeros(B, ld, ld, dtype=dtype, device="cuda")
    H[:, :n, :n] = torch.tril(M)
    Hnan = H.clone()
    Hnan[:, :n, :n] += torch.triu(torch.full((n, n), float("nan"), dtype=dtype, device="cuda"), 1)
    Hc = Hnan.clone()
    b = torch.randn(B, n, dtype=F64, device="cuda", generator=_gen(B)).to(dtype)
    lam = None if damping is None else torch.linspace(0.02, 0.3, B, dtype=F64, device="cuda").to(dtype)
    ell, eps = damping == "ellipsoidal", 1e-6
    LU, piv, info, _, x = _lu_n(_K(), Hnan, n, lam, ell, eps, True, b, None)
    assert torch.equal(torch.nan_to_num(Hnan, nan=7.0), torch.nan_to_num(Hc, nan=7.0))     # (the source is read only)
    assert info.cpu().tolist() == [0] * B
    sym = torch.tril(M) + torch.tril(M, -1).transpose(1, 2)
    _check_against_lapack(_damped(sym, lam, ell, eps), LU, piv, x, b, dtype, sorted({0, B // 2, B - 1}), f"spd-{damping}")
    _, xc, ic = factor_and_solve(_K(), H, n, b, damping=lam, ellipsoidal=ell, eps=eps)
    torch.cuda.synchronize()
    assert int(ic.abs().sum()) == 0
    tol_x = 2e-3 if dtype == F32 else 1e-10
    assert float((x - xc).abs().max() / xc.abs().max()) < tol_x


# ---- 3. what the Cholesky cannot do ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [6, 130])
def test_symmetric_indefinite_with_zero_diagonal(n, dtype):
    """[[0, C], [C^T, 0]] with a well-conditioned C (orthogonal times diag(1 ... 2)): thx_chol_factor reports a failure,
    thx_lu_factor does not, and its solution meets the bar of the tests above."""
    from tests.gpu_helpers import factor_and_solve
    B, m = 3, n // 2
    g = _gen(n)
    Q = torch.linalg.qr(torch.randn(B, m, m, dtype=F64, device="cuda", generator=g)).Q
    C = Q * torch.linspace(1.0, 2.0, m, dtype=F64, device="cuda")
    M = torch.zeros(B, n, n, dtype=F64, device="cuda")
    M[:, :m, m:] = C
    M[:, m:, :m] = C.transpose(1, 2)
    M = M.to(dtype)
    M = torch.tril(M) + torch.tril(M, -1).transpose(1, 2)          # (exactly symmetric after rounding)
    b = torch.randn(B, n, dtype=F64, device="cuda", generator=g).to(dtype)
    ld = _ld(n)
    H = torch.zeros(B, ld, ld, dtype=dtype, device="cuda")
    H[:, :n, :n] = torch.tril(M)
    _, _, ic = factor_and_solve(_K(), H, n, b)
    torch.cuda.synchronize()
    assert (ic != 0).all(), ic
    for sym_mode, src in ((True, H), (False, M.contiguous())):
        LU, piv, info, _, x = _lu_n(_K(), src, n, None, False, 1e-8, sym_mode, b, None)
        assert info.cpu().tolist() == [0] * B
        _check_against_lapack(M, LU, piv, x, b, dtype, range(B), "indefinite")


# ---- 4. singularity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,dtype", [(40, 35, F64), (70, 40, F32), (24, 9, F32)])
def test_singular_item_is_reported_as_lapack_does(n, k, dtype):
    """Item 1 of 3 is exactly singular at column k: integer entries, block upper triangular with a leading (k + 1) x (k + 1) block
    that holds two identical rows.  Their first entry dominates column 0, so step 0 takes one as the pivot row and subtracts it
    from the other with a multiplier of exactly 1: a zero row, in any order of arithmetic.  It is passed over until column k, where
    nothing else is left in the leading block."""
    g = _gen(n)
    M = torch.randint(-9, 10, (3, n, n), device="cuda", generator=g).to(dtype)
    M[1, k + 1:, :k + 1] = 0
    M[1, k] = M[1, 2]
    M[1, 2, 0] = M[1, k, 0] = 50
    b = torch.randn(3, n, dtype=F64, device="cuda", generator=g).to(dtype)
    expect = torch.linalg.lu_factor_ex(M.cpu()).info.tolist()
    assert expect == [0, k + 1, 0]                                   # (the premise, by LAPACK alone)
    LU, piv, info, _, x = _lu(M, rhs=b, fill=0.0)
    assert info.cpu().tolist() == expect
    keep = [0, 2]
    LU2, piv2, info2, _, x2 = _lu(M[keep].contiguous(), rhs=b[keep].contiguous(), fill=0.0)
    assert info2.cpu().tolist() == [0, 0]
    assert torch.equal(LU[keep], LU2) and torch.equal(piv[keep], piv2) and torch.equal(x[keep], x2)


def _zero_weight_objective(th):
    from tests.test_gpu_lm import build_objective
    g = dict(load_golden("pg_f64_gn"))
    g["w_between"] = g["w_between"] * 0.0
    g["w_prior"] = g["w_prior"] * 0.0
    return build_objective(th, g)[0]


def test_singular_system_raises_and_fails_the_loop():
    """All weights zero: AtA = 0.  HipLUSolver.solve() raises torch.linalg.solve's error, the LM loop ends with FAIL status, as it
    does for a failed Cholesky (tests/test_gpu_lm.py:test_non_positive_definite_sets_fail_status)."""
    import warnings
    import theseus_amd as th
    obj = _zero_weight_objective(th)
    opt = th.LevenbergMarquardt(obj, linear_solver_cls=th.HipLUSolver, max_iterations=3)
    obj.update()
    opt.linear_solver.linearization.linearize()
    with pytest.raises(RuntimeError, match=r"linalg\.solve: \(Batch element 0\): The solver failed because the input matrix is singular\."):
        opt.linear_solver.solve(damping=None)
    assert int(opt.linear_solver.info[0]) == 1
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        info = opt.optimize(damping=0.0, ellipsoidal_damping=False)
    assert all(s == th.NonlinearOptimizerStatus.FAIL for s in info.status)


# ---- 5. stale buffers --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,B,dtype,sym", [(33, 3, F32, False), (129, 3, F64, True), (200, 65, F32, True)])
def test_results_do_not_depend_on_stale_buffers(n, B, dtype, sym):
    g = _gen(n)
    A = torch.randn(B, n, n, dtype=F64, device="cuda", generator=g)
    M = (A @ A.transpose(1, 2) / n if sym else A).to(dtype)
    if sym:
        ld = _ld(n)
        H = torch.zeros(B, ld, ld, dtype=dtype, device="cuda")
        H[:, :n, :n] = torch.tril(M)
        M = H
    b = torch.randn(B, n, dtype=F64, device="cuda", generator=g).to(dtype)
    lam = torch.linspace(0.1, 0.2, B, dtype=F64, device="cuda").to(dtype)
    outs = [_lu_n(_K(), M, n, lam, True, 1e-6, sym, b, fill) for fill in (float("nan"), 0.0)]
    for a, c in zip(*outs):
        assert torch.equal(a, c)
    assert not torch.isnan(outs[0][0]).any() and not torch.isnan(outs[0][4]).any()


# ---- 6. end to end on the fixtures of the Cholesky solver's tests ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pg_f64_lm", "pg_f64_lm_adaptive_ellips", "pg2_f64_lm"])
def test_lm_trajectory_with_the_lu_solver(name):
    """tests/test_gpu_lm.py:test_lm_trajectory_matches_reference with linear_solver_cls=HipLUSolver: same arrays, same tolerances."""
    import theseus_amd as th
    from tests.test_gpu_lm import build_objective, well_conditioned_steps
    tol = 1e-7
    g = load_golden(name)
    _, _, kw = golden_problem(g)
    obj, poses = build_objective(th, g)
    assert not kw.pop("gauss_newton", False)
    okw = dict(max_iterations=kw.pop("max_iterations"), step_size=kw.pop("step_size"), abs_err_tolerance=0.0, rel_err_tolerance=0.0)
    opt = th.LevenbergMarquardt(obj, linear_solver_cls=th.HipLUSolver, **okw)
    assert isinstance(opt.linear_solver, th.HipLUSolver)
    deltas = []
    sol, info = th.TheseusLayer(opt).forward(None, optimizer_kwargs=dict(
        track_err_history=True, end_iter_callback=lambda o, i, d, it: deltas.append(d.clone()), **kw))
    final = torch.stack([sol[f"pose_{k}"] for k in range(int(g["P"]))], 1).cpu().numpy()
    ok = well_conditioned_steps(g, g["delta"].shape[0])
    slack = 2.0 * (np.abs(g["delta"]).max(axis=2) * ~ok).sum(axis=0)
    assert (np.abs(final - g["final"]).reshape(final.shape[0], -1).max(1) <= tol + slack).all()
    if len(deltas) == g["delta"].shape[0]:
        for it, d in enumerate(deltas):
            np.testing.assert_allclose(d.cpu().numpy()[ok[it]], g["delta"][it][ok[it]], rtol=0,
                                       atol=tol * max(1.0, np.abs(g["delta"][it]).max()))
    k = min(info.err_history.shape[1], g["err_history"].shape[1])
    np.testing.assert_allclose(info.err_history[:, :k].numpy(), g["err_history"][:, :k], rtol=2e-5)
    assert all(s == th.NonlinearOptimizerStatus.MAX_ITERATIONS for s in info.status)


def test_implicit_gradients_with_the_lu_solver():
    import theseus_amd as th
    from tests.implicit_common import check_against_reference, run_implicit
    g = load_golden("pg_f64_implicit")
    final, loss, grads, info, _, _ = run_implicit(th, g, "cuda", solver=dict(linear_solver_cls=th.HipLUSolver))
    check_against_reference(g, final, loss, grads)


def test_unrolled_gradients_with_the_lu_solver():
    import theseus_amd as th
    from tests.unrolled_common import run_pg_unrolled
    run_pg_unrolled(th, load_golden("pg_f64_unrolled"), "gn_unroll", "cuda", solver_cls=th.HipLUSolver)


class _WithLU:
    """theseus_amd with the LU solver as the optimizers' linear solver (tests/simple_example_common.py picks no solver itself)."""

    def __init__(self, th):
        self._th = th

    def __getattr__(self, name):
        attr = getattr(self._th, name)
        if name in ("GaussNewton", "LevenbergMarquardt"):
            return lambda *a, **k: attr(*a, linear_solver_cls=self._th.HipLUSolver, **k)
        return attr


def test_simple_example_with_the_lu_solver():
    """The generic path (thx_block_assemble's frame, symmetric-lower mode) against tests/golden/simple_example.npz."""
    import theseus_amd as th
    from tests.simple_example_common import check_simple_example, run_simple_example
    g = load_golden("simple_example")
    r = run_simple_example(_WithLU(th), g, "cuda")
    assert isinstance(r["opt"].linear_solver, th.HipLUSolver) and isinstance(r["opt2"].linear_solver, th.HipLUSolver)
    check_simple_example(g, r)
