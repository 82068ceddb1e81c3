"""-m gpu: HipCholeskySolver(ordering="auto") -- the dense solver factorises a block-compact linearization in the order of
thx_hblock_order, inside its own layout; g, x and every tensor a caller sees stay in the linearization's order.

SE3 pose graphs (a chain plus random closures, four edges per pose) of 5, 6 and 7 block columns: 106 poses (n = 636), 107 poses
(n = 642: the sixth block column holds two rows) and 149 poses (n = 894).  The solves of "auto" and "natural" on the SAME
linearization are each compared with fp64 LAPACK on H + lambda diag(H) + eps; rounding differs with the order and nothing else does,
so "auto" may miss LAPACK by MARGIN times what "natural" misses it by on the same inputs.

MARGIN = 4.  Both errors are the forward error of a backward-stable Cholesky solve of one matrix: bounded by the same
c n eps cond(H), realised as sums of the same number of rounding terms whose signs depend on the summation order.  Two such draws
of the largest component over 600 - 900 unknowns and 8 - 11 problems differ by far less than a factor of four; a lost block, a wrong
transposition or a mis-gathered vector is an error of order one.  Measured "natural" error (max over problems of
max |x - x_lapack| / max |x_lapack|) on the 149-pose graph at batch 11: fp32 3.95e-5, fp64 1.24e-13; "auto" on the same inputs:
fp32 3.26e-5, fp64 1.63e-13 (over all graphs and batches: fp32 2.9e-5 ... 4.6e-5 against 3.1e-5 ... 4.0e-5, fp64 1.2e-13 ...
1.6e-13 against 1.6e-13 ... 1.7e-13)."""
import functools

import pytest
import torch

from tests.test_gpu_zero_block_skip import GATHER, _kernels

pytestmark = pytest.mark.gpu

MARGIN = 4.0
GRAPHS = {"p106": (106, 5), "p107": (107, 6), "p149": (149, 7)}
DTYPES = {"f32": torch.float32, "f64": torch.float64}
LAM = 1e-3


def _edges(name):
    from theseus_amd.utils import synthetic as syn
    if name == "chain107":
        return [(k - 1, k) for k in range(1, 107)], 107
    P = GRAPHS[name][0]
    return syn.pose_graph_topology(P, 4 * P, topology_seed=0), P


@functools.lru_cache(maxsize=None)
def _objective(name, dtype):
    from theseus_amd.utils import synthetic as syn
    edges, P = _edges(name)
    return syn.build_pose_graph_objective(edges, P, dtype=DTYPES[dtype], device="cuda"), edges, P


def _solvers(name, dtype, B, Ks, seed=99):
    """("auto" solver, "natural" solver) on one objective and one kernels object, both linearized at the same random poses."""
    import theseus_amd as th
    from theseus_amd.utils import synthetic as syn
    obj, edges, P = _objective(name, dtype)
    obj.update(syn.input_dict(syn.make_pose_graph_tensors(edges, P, B, dtype=DTYPES[dtype], device="cuda", seed=seed)))
    out = []
    for ordering in ("auto", "natural"):
        s = th.HipCholeskySolver(obj, linearization_kwargs=dict(kernels=Ks), ordering=ordering)
        s.linearization.linearize()
        assert s.linearization._compact
        out.append(s)
    return out


def _lapack(lin, lam=LAM, eps=1e-8):
    """fp64 LAPACK on the system the solvers damp ellipsoidally: (H + lam diag(H) + eps) x = g, on the host."""
    H = lin.AtA.double().cpu()
    d = torch.diagonal(H, dim1=1, dim2=2)
    M = H + torch.diag_embed(lam * d + eps)
    return torch.cholesky_solve(lin.g.double().cpu().unsqueeze(2), torch.linalg.cholesky(M)).squeeze(2)


def _err(x, want):
    x = x.double().cpu()
    return float(((x - want).abs().amax(dim=1) / want.abs().amax(dim=1)).max())


def _schedule(gather, split_min, dtype):
    # the left-looking schedule at these batch sizes, column pairs on in fp32 (thx_chol_schedule; tests/test_gpu_tile_sorted_rows.py)
    return _kernels(split_diag_min_batch=split_min, hb_scatter_max_pieces=GATHER[gather], right_looking_max_batch=0,
                    column_pairs_min_batch=0, column_pairs=1)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("gather", list(GATHER))
@pytest.mark.parametrize("B,split_min", [(11, 2 ** 31 - 1), (8, 0)], ids=["b11", "b8split"])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_auto_and_natural_against_lapack(name, B, split_min, gather, dtype):
    Ks = _schedule(gather, split_min, dtype)
    auto, nat = _solvers(name, dtype, B, Ks)
    n = auto.linearization.n
    assert (n + 127) // 128 == GRAPHS[name][1]
    p = Ks.chol_plan(n, auto.linearization.ld, B, DTYPES[dtype], damping=True, rhs=True, ldv=n, layout=auto._ordered()[0].c)
    assert p["right_looking"] == 0 and p["split_diag"] == int(B >= split_min), p
    if dtype == "f32":
        # the permuted layout keeps the structure-aware paths (five block columns: one tile below pair 2, which begins at chunk 0 in
        # either order -- pair 0's groups and the zero solves only)
        rg = auto._ordered()[0].host.row_groups()
        assert p["column_pairs"] == 1 and p["skip_zero_solves"] == 1 and p["regroup_rows"] == int(rg.ngroups > 0), p
        assert rg.ngroups0 > 0 and (rg.ngroups > 0) == (name != "p106")
    xa, xn = auto.solve(damping=LAM), nat.solve(damping=LAM)
    assert auto._factor_ord is not None and nat._factor_ord is None
    assert auto._factor_ord[0].host.nblocks == nat.linearization.hblocks.host.nblocks
    assert torch.equal(auto.linearization.Hc, nat.linearization.Hc) and torch.equal(auto.linearization.g, nat.linearization.g)
    want = _lapack(nat.linearization)
    ea, en = _err(xa, want), _err(xn, want)
    print(f"{name} B={B} {gather} {dtype}: natural {en:.3e} auto {ea:.3e}")
    assert torch.isfinite(xa).all() and en > 0
    assert en < (2e-3 if dtype == "f32" else 1e-11), en                  # (the yardstick itself is a solve)
    assert ea <= MARGIN * en, (ea, en)


def test_structural_zeros_of_the_permuted_factor_on_a_nan_filled_frame():
    """L of P H P^T is zero left of the permuted layout's row_first and finite from there to the diagonal: the frame is filled with
    NaN before the factorisation, so an element the kernels should have stored and did not shows."""
    Ks = _schedule("mfma", 0, "f32")
    auto, _ = _solvers("p149", "f32", 8, Ks)
    auto.solve(damping=LAM)                                   # (allocates the frame)
    auto._L.fill_(float("nan"))
    x = auto.solve(damping=LAM)
    n = auto.linearization.n
    L = auto._L[:, :n, :n]
    first = auto._factor_ord[0].t["row_first"].long()
    cols = torch.arange(n, device="cuda")
    left = cols[None, :] < first[:, None]
    inside = (cols[None, :] >= first[:, None]) & (cols[None, :] <= cols[:, None])
    assert left.any() and float(left.sum()) > 0.2 * n * n / 2          # the permuted envelope leaves out a good part of the triangle
    assert (L[:, left] == 0).all()
    assert torch.isfinite(L[:, inside]).all() and torch.isfinite(x).all()
    # and the order really differs from the insertion order's envelope
    nat_first = auto.linearization.hblocks.t["row_first"].long()
    assert not torch.equal(first, nat_first)


def test_a_chain_keeps_the_insertion_order():
    Ks = _schedule("mfma", 2 ** 31 - 1, "f32")
    auto, nat = _solvers("chain107", "f32", 8, Ks)
    assert auto._ordered() is None
    xa, xn = auto.solve(damping=LAM), nat.solve(damping=LAM)
    assert auto._factor_ord is None and torch.equal(xa, xn) and torch.equal(auto.L, nat.L)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_solves_on_the_cached_factor_stay_in_the_linearizations_order(dtype):
    """solve_with_factor, a snapshot, one multi-right-hand-side solve and the marginal covariance on a factor made in the solver's
    own order, each against fp64 LAPACK and against the natural order's error on the same inputs."""
    Ks = _schedule("mfma", 2 ** 31 - 1, dtype)
    auto, nat = _solvers("p107", dtype, 8, Ks)
    lin = nat.linearization
    n, dt = lin.n, DTYPES[dtype]
    H = lin.AtA.double().cpu()
    d = torch.diagonal(H, dim1=1, dim2=2)
    M = H + torch.diag_embed(LAM * d + 1e-8)
    chol = torch.linalg.cholesky(M)
    gen = torch.Generator("cuda").manual_seed(8)
    rhs = torch.randn(8, n, dtype=dt, device="cuda", generator=gen)
    for s in (auto, nat):
        s.solve(damping=LAM)
    assert auto._factor_ord is not None
    want = torch.cholesky_solve(rhs.double().cpu().unsqueeze(2), chol).squeeze(2)
    ea, en = _err(auto.solve_with_factor(rhs), want), _err(nat.solve_with_factor(rhs), want)
    print(dtype, "solve_with_factor: natural", en, "auto", ea)
    assert en > 0 and ea <= MARGIN * en, (ea, en)
    snap_a, snap_n = auto.factor_snapshot(), nat.factor_snapshot()
    # multi-right-hand-side: 33 vectors (two groups of 32), H^-1 and the two halves composed
    R = torch.randn(8, 33, n, dtype=dt, device="cuda", generator=gen)
    wantR = torch.cholesky_solve(R.double().cpu().transpose(1, 2), chol).transpose(1, 2)
    relm = lambda X: float((X.double().cpu() - wantR).abs().amax() / wantR.abs().amax())   # noqa: E731
    ea, en = relm(auto.solve_multi_with_factor(R)), relm(nat.solve_multi_with_factor(R))
    print(dtype, "solve_multi_with_factor: natural", en, "auto", ea)
    assert en > 0 and ea <= MARGIN * en, (ea, en)
    eh = relm(auto.solve_multi_with_factor(auto.solve_multi_with_factor(R, which=2), which=1))
    assert eh <= MARGIN * en, (eh, en)
    # a later factorisation leaves the snapshots valid, each in the order it was made in
    for s in (auto, nat):
        s.solve(damping=10 * LAM)
    ea, en = _err(auto.solve_with_snapshot(snap_a, rhs), want), _err(nat.solve_with_snapshot(snap_n, rhs), want)
    assert en > 0 and ea <= MARGIN * en, (ea, en)
    # the frame a caller reads is the factor in the linearization's order: L L^T = H + 10 lam diag(H) + eps
    M10 = (H + torch.diag_embed(10 * LAM * d + 1e-8))
    La = torch.tril(auto.L[:, :n, :n]).double().cpu()
    resid = float((La @ La.transpose(1, 2) - M10).abs().max() / M10.abs().max())
    assert resid < (1e-5 if dtype == "f32" else 1e-13), resid
    # marginal covariance of two variables, in the order asked for (fp64 only: the factor is undamped and the graph hangs on one
    # prior, cond(H) ~ 1e9 -- fp32 has no digits of H^-1 to compare in either order)
    if dtype == "f32":
        return
    names = [v.name for v in auto.linearization.ordering]
    pick = [names[40], names[3]]
    Ca, Cn = auto.marginal_covariance(pick), nat.marginal_covariance(pick)
    assert auto._factor_ord is not None
    idx = torch.tensor(list(range(240, 246)) + list(range(18, 24)))
    wantC = torch.linalg.inv(H)[:, idx][:, :, idx]
    relc = lambda C: float((C.double().cpu() - wantC).abs().amax() / wantC.abs().amax())   # noqa: E731
    ea, en = relc(Ca), relc(Cn)
    print(dtype, "marginal_covariance: natural", en, "auto", ea)
    assert en > 0 and ea <= MARGIN * en, (ea, en)


def test_a_short_lm_run_ends_at_the_natural_orders_cost():
    """Three LM iterations in fp32 with "auto" and with "natural", and the same run in fp64 ("natural") as the yardstick: the final
    cost of "auto" may miss the fp64 one by MARGIN times what "natural" misses it by -- or by 16 fp32 roundings of the cost, which
    is a sum of ~3600 squared residuals evaluated in fp32 and can land on the fp64 value by chance."""
    import theseus_amd as th
    from theseus_amd.utils import synthetic as syn
    edges, P = _edges("p149")
    B = 8
    cost = {}
    for key, dt, ordering in (("auto", torch.float32, "auto"), ("natural", torch.float32, "natural"), ("ref", torch.float64, "natural")):
        obj = syn.build_pose_graph_objective(edges, P, dtype=dt, device="cuda")
        opt = th.LevenbergMarquardt(obj, linear_solver_cls=th.HipCholeskySolver, linear_solver_kwargs=dict(ordering=ordering),
                                    max_iterations=3, abs_err_tolerance=0.0, rel_err_tolerance=0.0, step_size=1.0)
        inputs = syn.input_dict(syn.make_pose_graph_tensors(edges, P, B, dtype=torch.float64, device="cuda", seed=99))
        inputs = {k: v.to(dt) for k, v in inputs.items()}
        _, info = th.TheseusLayer(opt).forward(inputs, optimizer_kwargs=dict(damping=LAM, track_err_history=True))
        assert (opt.linear_solver._factor_ord is not None) == (ordering == "auto")
        cost[key] = info.err_history[:, -1].double().cpu()
        assert (info.err_history[:, -1] < info.err_history[:, 0]).all()
    ea = ((cost["auto"] - cost["ref"]).abs() / cost["ref"]).max()
    en = ((cost["natural"] - cost["ref"]).abs() / cost["ref"]).max()
    print("final cost against fp64: natural", float(en), "auto", float(ea))
    assert float(ea) <= MARGIN * max(float(en), 16 * 2.0 ** -24), (float(ea), float(en))
