"""-m gpu: the dense-frame triangular solves reading only the row envelope of L (thx_chol_solve_env / thx_chol_solve_backward_env,
thx_hblock_layout.row_first).  The envelope kernels leave out loads and products left of row_first[r] and keep every sum's order,
so what they trust is checked first -- every schedule of thx_chol_factor_hblocks stores exact zeros there, into a frame pre-filled
with NaN -- and then x must be the same with and without the table (torch.equal: -0 and +0 are equal), in fp32 and fp64.

Graphs (zero share of the strictly-lower tiles left of row_first, 16-byte granularity): 48 poses / 96 edges (n = 288, three block
rows, 32 rows in the last tile, 63 %), 70 / 140 with topology seed 1 (n = 420, four block rows, 36 rows in the last, 60 %), a pure
chain of 70 poses (row_first one pose back: the most is skipped) and a star of 48 poses on pose 0 (row_first = 0: nothing is)."""
import functools

import numpy as np
import pytest
import torch

from tests.test_solve_envelope_host import layout

pytestmark = pytest.mark.gpu

GRAPHS = ["p48", "p70", "path70", "star48"]
DTYPES = {"f32": torch.float32, "f64": torch.float64}
B = 40          # above the 32 problems that the block-row kernel serves: chol_bwd_kernel is reached
B_SMALL = 8     # the block-row kernel; the right-looking schedule's batch


def _kernels(**fields):
    from theseus_amd.kernels import HipKernels
    Ks = HipKernels()
    for k, v in fields.items():
        setattr(Ks.chol_schedule, k, v)
    return Ks


def _factor_nan(Ks, dhb, Hc, n, rhs):
    """thx_chol_factor_hblocks into an L frame pre-filled with NaN -> (L, panels, y)."""
    nb, dt = Hc.shape[0], Hc.dtype
    nt = (n + 127) // 128
    lam = torch.full((nb,), 1e-3, dtype=dt, device="cuda")
    L = torch.full((nb, nt * 128, nt * 128), float("nan"), dtype=dt, device="cuda")
    panels = torch.zeros(nb, nt, 128, 128, dtype=dt, device="cuda")
    info = torch.empty(nb, dtype=torch.int32, device="cuda")
    y = torch.empty_like(rhs)
    Ks.chol_factor_hblocks(dhb, Hc, n, lam, False, 1e-8, L, panels, info, rhs=rhs, y=y)
    assert int(info.abs().sum()) == 0
    return L, panels, y


@functools.lru_cache(maxsize=None)
def _case(graph, dtype):
    """One random SPD system per (graph, precision) with exactly the layout's block pattern, factorised once at batch 40 with the
    default schedule; shared by the tests below, which leave it unchanged."""
    hb = layout(graph)
    n, dt = hb.bd * hb.nvars, DTYPES[dtype]
    rng = np.random.default_rng(5)
    H = np.zeros((B, n, n))
    for a, b in hb.blocks.tolist():
        H[:, 6 * a:6 * a + 6, 6 * b:6 * b + 6] = rng.standard_normal((B, 6, 6))
    H = np.tril(H, -1)
    H = H + H.transpose(0, 2, 1)
    idx = np.arange(n)
    H[:, idx, idx] = np.abs(H).sum(2) + 1.0 + rng.random((B, n))
    Hc = torch.from_numpy(hb.pack_dense(np.tril(H))).to(dt).cuda()
    rhs = torch.randn(B, n, dtype=dt, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    dhb = hb.on("cuda")
    Ks = _kernels()
    L, panels, y = _factor_nan(Ks, dhb, Hc, n, rhs)
    return dict(hb=hb, dhb=dhb, n=n, dt=dt, Hc=Hc, rhs=rhs, L=L, panels=panels, y=y, K=Ks, first=dhb.t["row_first"])


def _assert_zero_left_of_first(L, first, n):
    """L[:, r, :first[r]] == 0 for every row (exact zeros of either sign: NaN, the pre-fill, fails), and a finite lower triangle."""
    cols = torch.arange(n, device="cuda")
    left = cols[None, :] < first[:n, None].to(torch.int64)
    Ln = L[:, :n, :n]
    assert bool((Ln[:, left] == 0).all())
    assert bool(torch.isfinite(Ln[:, cols[:, None] >= cols[None, :]]).all())


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("graph", GRAPHS)
def test_every_schedule_stores_exact_zeros_left_of_row_first(graph, dtype):
    c = _case(graph, dtype)
    n, dt, dhb, first = c["n"], c["dt"], c["dhb"], c["first"]
    ld = (n + 127) // 128 * 128
    _assert_zero_left_of_first(c["L"], first, n)           # batch 40, the default schedule
    Hc, rhs = c["Hc"][:B_SMALL].contiguous(), c["rhs"][:B_SMALL].contiguous()
    left = _kernels(right_looking_max_batch=0, column_pairs_min_batch=0, column_pairs=1)
    right = _kernels(right_looking_max_batch=B_SMALL)
    pl = left.chol_plan(n, ld, B_SMALL, dt, damping=True, rhs=True, ldv=rhs.stride(0), layout=dhb.c)
    pr = right.chol_plan(n, ld, B_SMALL, dt, damping=True, rhs=True, ldv=rhs.stride(0), layout=dhb.c)
    assert pl["right_looking"] == 0 and pl["column_pairs"] == int(dt == torch.float32), pl   # (the pairs are the fp32 schedule)
    assert pr["right_looking"] == 1, pr
    for Ks in (left, right):
        L8, _, _ = _factor_nan(Ks, dhb, Hc, n, rhs)
        _assert_zero_left_of_first(L8, first, n)


def _solve(c, mode, table):
    """x of one solve on the shared factor: 'backward' (x = L^-T y), 'both' ((L L^T)^-1 rhs), 'alias' (backward, x aliasing y)."""
    K, n, rf = c["K"], c["n"], (c["first"] if table else None)
    if mode == "both":
        x = torch.full_like(c["rhs"], float("nan"))
        K.chol_solve(c["L"], n, c["panels"], c["rhs"], x, row_first=rf)
    elif mode == "backward":
        x = torch.full_like(c["y"], float("nan"))
        K.chol_solve_backward(c["L"], n, c["panels"], c["y"], x, row_first=rf)
    else:
        x = c["y"].clone()
        K.chol_solve_backward(c["L"], n, c["panels"], x, x, row_first=rf)
    return x


@pytest.mark.parametrize("mode", ["backward", "both", "alias"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("graph", GRAPHS)
def test_envelope_solve_is_bit_identical(graph, dtype, mode):
    c = _case(graph, dtype)
    x_env, x_all = _solve(c, mode, True), _solve(c, mode, False)
    assert bool(torch.isfinite(x_all).all()) and float(x_all.abs().max()) > 0
    assert torch.equal(x_env, x_all)
    if mode == "both":   # and it is a solution: L L^T x = rhs to the precision's rounding (diagonally dominant H, condition ~ 1e2)
        Lt = torch.tril(c["L"][:, :c["n"], :c["n"]]).double()
        res = (Lt @ (Lt.transpose(1, 2) @ x_env.double().unsqueeze(2))).squeeze(2) - c["rhs"].double()
        assert float(res.abs().max()) < (1e-3 if c["dt"] == torch.float32 else 1e-11) * float(c["rhs"].abs().max())


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("graph", GRAPHS)
def test_block_row_kernel_matches_the_envelope_kernel(graph, dtype):
    """Batch 8 goes to chol_bwd_rows_kernel (which reads every tile in full, table or not); its x equals the envelope kernel's at
    batch 40 on the same problems."""
    c = _case(graph, dtype)
    assert (c["n"] + 127) // 128 >= 3     # (the block-row kernel's floor)
    x40 = _solve(c, "backward", True)
    L8, P8, y8 = c["L"][:B_SMALL].contiguous(), c["panels"][:B_SMALL].contiguous(), c["y"][:B_SMALL].contiguous()
    for rf in (c["first"], None):
        x8 = torch.full_like(y8, float("nan"))
        c["K"].chol_solve_backward(L8, c["n"], P8, y8, x8, row_first=rf)
        assert torch.equal(x8, x40[:B_SMALL])


def test_lm_run_is_the_same_with_and_without_the_table():
    """Three LM iterations of the 48-pose graph at batch 40 with the solver passing the layout's table and passing nothing: the
    solved poses and the error history are the same."""
    import theseus_amd as th
    from theseus_amd.utils import synthetic as syn
    edges = syn.pose_graph_topology(48, 96, 0)
    res = []
    for env in (True, False):
        obj = syn.build_pose_graph_objective(edges, 48, dtype=torch.float32, device="cuda")
        opt = th.LevenbergMarquardt(obj, linear_solver_cls=th.HipCholeskySolver, max_iterations=3, abs_err_tolerance=0.0,
                                    rel_err_tolerance=0.0, step_size=1.0)
        solver = opt.linear_solver
        solver.solve_envelope = env
        seen = []
        inner = solver.K.chol_solve_backward
        solver.K.chol_solve_backward = lambda *a, **k: (seen.append(k.get("row_first")), inner(*a, **k))[1]
        try:
            inputs = syn.input_dict(syn.make_pose_graph_tensors(edges, 48, B, dtype=torch.float32, device="cuda", seed=99))
            sol, info = th.TheseusLayer(opt).forward(inputs, optimizer_kwargs=dict(damping=1e-3, track_err_history=True))
        finally:
            del solver.K.chol_solve_backward   # (the instance attribute: the method is the class's again)
        assert len(seen) >= 3 and all((t is not None) == env for t in seen)   # the path under test was taken
        res.append((torch.stack([sol[f"VERTEX_SE3__{k}"] for k in range(48)], 1), info.err_history))
    assert bool(torch.isfinite(res[0][0]).all())
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])
