"""-m gpu: thx_chol_solve_multi_sparse (csrc/sparse_multi_kernels.hip) -- triangular solves with a block of right-hand sides on the
tile-sparse Cholesky factor, and HipSparseCholeskySolver's solve_multi_with_factor / sample_deltas / marginal_covariance on it.
Part 1: the kernel on the factor of block-banded matrices (absent tiles, fill, a last tile of 6 rows), dense frame and tile-packed,
with NaN wherever it must not read, against the fp64 substitution on the device's own L (bars of tests/test_gpu_multi_solve.py).
Part 2: the solver's three layouts on a 120-pose chain graph against fp64 on the CPU."""
import pytest
import torch

from tests.test_gpu_multi_solve import BAR, F32, F64, _check, _reference, _rhs
from tests.test_gpu_sampling import reference_delta_samples, relerr
from tests.test_gpu_sparse import _banded_spd, _chain_problem

pytestmark = pytest.mark.gpu
B, NAN = 3, float("nan")
_FACTORS, _SOLVERS = {}, {}


def _factored(n, dtype):
    """{"frame": L, "packed": L}, panels, pattern, L as fp64 on the host -- factorised once per (n, dtype), then poisoned."""
    if (n, dtype) not in _FACTORS:
        from theseus_amd.kernels import default_kernels, round_up
        H, pat = _banded_spd(B, n, 1, dtype, seed=n)
        nt, ld = pat.ntiles, round_up(n, 32)
        assert pat.l_tiles < nt * (nt + 1) // 2
        Hf = torch.zeros(B, ld, ld, dtype=dtype, device="cuda")
        Hf[:, :n, :n] = H.cuda()
        L, panels = torch.zeros_like(Hf), torch.empty(B, nt, 128, 128, dtype=dtype, device="cuda")
        info = torch.empty(B, dtype=torch.int32, device="cuda")
        default_kernels().chol_factor_sparse(Hf, n, None, False, 1e-8, L, panels, info, pat)
        assert int(info.abs().sum()) == 0
        L64 = torch.tril(L[:, :n, :n].double().cpu())
        packed = torch.zeros(B, pat.nslots, 128, 128, dtype=dtype, device="cuda")
        L[:, n:, :] = NAN                                      # the frame's padding rows
        last = n - 128 * (nt - 1)
        for i in range(nt):
            for j in range(nt):
                r0, c0, r1, c1 = 128 * i, 128 * j, min(128 * i + 128, ld), min(128 * j + 128, ld)
                if (i, j) not in pat.slot:
                    L[:, r0:r1, c0:c1] = NAN                   # tiles outside the pattern
                    continue
                s = pat.slot[(i, j)]
                packed[:, s, :r1 - r0, :c1 - c0] = L[:, r0:r1, c0:c1]
                if i == nt - 1:
                    packed[:, s, last:, :] = NAN               # unused rows of the last block row's slots ...
                    if j == i:
                        packed[:, s, :, last:] = NAN           # ... and unused columns of the last tile
        _FACTORS[(n, dtype)] = (dict(frame=L, packed=packed), panels, pat, L64)
    return _FACTORS[(n, dtype)]


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("layout", ["frame", "packed"])
@pytest.mark.parametrize("nrhs,which", [(1, 0), (5, 1), (32, 2), (33, 0), (70, 0)])
@pytest.mark.parametrize("n", [390, 774])
def test_kernel_against_fp64_substitution_with_the_devices_factor(n, nrhs, which, layout, dtype):
    from theseus_amd.kernels import default_kernels
    Ls, panels, pat, L64 = _factored(n, dtype)
    rhs = _rhs(n, nrhs, dtype).cuda()
    keep = rhs.clone()
    x = torch.full_like(rhs, NAN)                              # (the result does not depend on what x held)
    default_kernels().chol_solve_multi_sparse(Ls[layout], n, panels, rhs, x, pat, which=which)
    assert torch.equal(rhs, keep)
    _check(x, _reference(L64, rhs, which), dtype, f"n={n} nrhs={nrhs} which={which} {layout}")


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("layout", ["frame", "packed"])
def test_in_place_on_strided_views_keeps_the_gaps(layout, dtype):
    from theseus_amd.kernels import default_kernels
    n, nrhs = 390, 33
    ldv, sentinel = n + 12, -12345.0
    bstride = nrhs * ldv + 40
    Ls, panels, pat, L64 = _factored(n, dtype)
    rhs = _rhs(n, nrhs, dtype, seed=9)
    buf = torch.full((B * bstride,), sentinel, dtype=dtype, device="cuda")
    xv = buf.as_strided((B, nrhs, n), (bstride, ldv, 1))
    xv.copy_(rhs.cuda())
    default_kernels().chol_solve_multi_sparse(Ls[layout], n, panels, xv, xv, pat, which=0)
    _check(xv, _reference(L64, rhs, 0), dtype, f"in place, strided, {layout}")
    written = torch.zeros(B * bstride, dtype=torch.bool, device="cuda")
    written.as_strided((B, nrhs, n), (bstride, ldv, 1)).fill_(True)
    assert bool((buf[~written] == sentinel).all())


# ---- the solver: tile-packed, dense frame, level schedule ----------------------------------------------------------------------------
LAYOUTS = dict(packed=dict(ordering="rcm", packed_factor=True), frame=dict(ordering="rcm", packed_factor=False), levels=dict(ordering="nd"))
# what HipCholeskySolver (dense frame) reaches on the same objective against the same fp64 references
# (profiles/sparse_multi/README.txt); the bars are four times that: the same kind of arithmetic in another elimination order
DENSE_COV = {F32: 1.88e-4, F64: 5.16e-13}       # (cond(AtA) of the three problems: 1.3e5 .. 1.8e5)
DENSE_SAMPLES = {F32: 1.88e-4, F64: 4.25e-13}


def _solver(layout, dtype):
    if (layout, dtype) not in _SOLVERS:
        import theseus_amd as th
        solver = _chain_problem(th, 120, B, dtype)(**LAYOUTS[layout]).linear_solver
        solver.linearization.linearize()
        _SOLVERS[(layout, dtype)] = solver
    return _SOLVERS[(layout, dtype)]


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_solver_blocks_samples_and_covariances(layout, dtype):
    solver = _solver(layout, dtype)
    lin, pat, n = solver.linearization, solver.pattern, 720
    assert solver.levels == (layout == "levels") and solver.packed_factor == (layout != "frame")
    if solver.levels:
        assert pat.tile_count.tolist() == [21, 21, 15, 21, 21, 21] and pat.tree_levels == 3
    solver.solve(damping=0.05)
    Ld = solver.dense_factor().double().cpu()
    keep = torch.from_numpy(pat.pad_of_col).long() if solver.levels else torch.arange(n)
    L64 = torch.tril(Ld[:, keep][:, :, keep])
    rhs = _rhs(n, 33, dtype, seed=23).cuda()
    for which in (0, 1, 2):
        _check(solver.solve_multi_with_factor(rhs, which), _reference(L64, rhs, which), dtype, f"{layout} which={which}")
    AtA = lin.AtA.double().cpu()
    cols = [c for name in ("pose_3", "pose_77") for k in [lin.ordering.index_of(name)]
            for c in range(lin.var_start_cols[k], lin.var_start_cols[k] + 6)]
    C = solver.marginal_covariance(["pose_3", "pose_77"])
    err = relerr(C, torch.linalg.inv(AtA)[:, cols][:, :, cols])
    print(layout, dtype, "marginal_covariance error", err)
    assert torch.equal(C, C.transpose(1, 2)) and err < 4 * DENSE_COV[dtype], err
    y = torch.randn(n, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(6)).to(dtype).cuda()
    samples = solver.sample_deltas(4, temperature=0.5, noise=y)
    err = relerr(samples, reference_delta_samples(AtA, solver.solve(), y, 0.5))
    print(layout, dtype, "sample_deltas error", err)
    assert err < 4 * DENSE_SAMPLES[dtype], err
