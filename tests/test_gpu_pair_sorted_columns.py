"""-m gpu: the fp32 column-pair kernel with the pair's 256 columns staged in ascending order of their first non-zero column
(thx_hblock_layout.sc_*, thx_chol_schedule.sort_pair_columns).  Every output element keeps its products in their order, what is left
out is a product with an exact zero, and the accumulators return to natural column order before anything else reads them: with the
switch on and off L, the solve panels, y and the solution must be the same (torch.equal: -0 and +0 are equal).  L is filled with NaN
before every factorisation: an element the kernel should have stored and did not is a NaN, not a stale value."""
import numpy as np
import pytest
import torch

from tests.test_gpu_zero_block_skip import GATHER, _kernels, _random_blocks
from tests.test_pair_columns_host import _graph

pytestmark = pytest.mark.gpu

# case -> (n, tile columns)
EXPECT = {"p90": (540, 5), "p128": (768, 6), "p140": (840, 7), "never140": (840, 7), "all0": (768, 6)}


def _factor_solve(Ks, dhb, Hc, n, B, rhs, row_first):
    nt = (n + 127) // 128
    ld = nt * 128
    lam = torch.full((B,), 1e-3, dtype=torch.float32, device="cuda")
    L = torch.full((B, ld, ld), float("nan"), dtype=torch.float32, device="cuda")
    panels = torch.zeros(B, nt, 128, 128, dtype=torch.float32, device="cuda")
    info = torch.empty(B, dtype=torch.int32, device="cuda")
    y = torch.empty_like(rhs)
    Ks.chol_factor_hblocks(dhb, Hc, n, lam, False, 1e-8, L, panels, info, rhs=rhs, y=y)
    assert int(info.abs().sum()) == 0
    x = torch.empty_like(rhs)
    Ks.chol_solve_backward(L, n, panels, y, x, row_first=row_first)
    return torch.tril(L[:, :n, :n]), panels, y, x


def _run(topo, split, gather, B):
    edges, P = _graph(topo)
    hb, dhb, Hc, n = _random_blocks(edges, P, B, seed=17)
    rg, pc = hb.row_groups(), hb.pair_columns()
    assert (n, hb.ntiles) == EXPECT[topo] and rg is not None and rg.group_ptr[2] > rg.group_ptr[1]   # pair j = 2 is regrouped
    assert 256 % 6 and 512 % 6                                   # a six-row variable straddles both edges of pair j = 2
    if topo == "all0":
        assert pc is None                                        # no table: the switch changes no launch
    else:
        assert pc.has[1] == 1 and pc.has.sum() == (2 if topo == "p140" else 1)      # p140: pairs j = 2 and j = 4
    if topo == "never140":
        assert (pc.first_chunk[1] >= 8).sum() == 7 and int(rg.k0[rg.group_ptr[1]]) == 0
    rhs = torch.randn(B, n, dtype=torch.float32, device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    out = []
    for sort in (1, 0):
        Ks = _kernels(split_diag_min_batch=0 if split else 2 ** 31 - 1, hb_scatter_max_pieces=GATHER[gather], right_looking_max_batch=0,
                      column_pairs_min_batch=0, column_pairs=1, skip_zero_blocks=1, regroup_rows=1, sort_pair_columns=sort)
        p = Ks.chol_plan(n, (n + 127) // 128 * 128, B, torch.float32, damping=True, rhs=True, ldv=rhs.stride(0), layout=dhb.c)
        assert p["right_looking"] == 0 and p["column_pairs"] == 1 and p["regroup_rows"] == 1, p
        assert p["sort_pair_columns"] == (sort if pc is not None else 0), p
        out.append(_factor_solve(Ks, dhb, Hc, n, B, rhs, dhb.t["row_first"]))
    (La, Pa, ya, xa), (Lb, Pb, yb, xb) = out
    assert torch.isfinite(La).all() and torch.isfinite(Lb).all() and La.abs().sum() > 0 and torch.isfinite(xa).all()
    assert torch.equal(La, Lb) and torch.equal(ya, yb) and torch.equal(xa, xb)
    for u in range(4):          # the ten lower sub-blocks of every panel (the others are never written)
        for v in range(u + 1):
            assert torch.equal(Pa[:, :, 32 * u:32 * u + 32, 32 * v:32 * v + 32], Pb[:, :, 32 * u:32 * u + 32, 32 * v:32 * v + 32])


@pytest.mark.parametrize("gather", list(GATHER))
@pytest.mark.parametrize("topo", list(EXPECT))
def test_sorting_the_pair_columns_leaves_the_factor_unchanged(topo, gather):
    _run(topo, False, gather, 8)


def test_sorted_pair_columns_with_the_split_diagonal_phase():
    _run("p140", True, list(GATHER)[0], 8)


def test_sorted_pair_columns_with_a_batch_that_is_no_multiple_of_eight():
    _run("p128", False, list(GATHER)[0], 11)


def test_sorting_the_pair_columns_leaves_the_lm_solution_unchanged():
    """Three LM iterations of the headline graph at 128 problems (the column-pair schedule's default floor) with the switch on and
    off: the solved poses and the error history are the same."""
    import theseus_amd as th
    from theseus_amd.utils import synthetic as syn
    edges = syn.pose_graph_topology(256, 1024, topology_seed=0)
    res = []
    for sort in (1, 0):
        obj = syn.build_pose_graph_objective(edges, 256, dtype=torch.float32, device="cuda")
        opt = th.LevenbergMarquardt(obj, linear_solver_cls=th.HipCholeskySolver, max_iterations=3, abs_err_tolerance=0.0,
                                    rel_err_tolerance=0.0, step_size=1.0)
        K = opt.linear_solver.K
        prev = K.chol_schedule.sort_pair_columns
        K.chol_schedule.sort_pair_columns = sort
        try:
            inputs = syn.input_dict(syn.make_pose_graph_tensors(edges, 256, 128, dtype=torch.float32, device="cuda", seed=99))
            sol, info = th.TheseusLayer(opt).forward(inputs, optimizer_kwargs=dict(damping=1e-3, track_err_history=True))
        finally:
            K.chol_schedule.sort_pair_columns = prev
        res.append((torch.stack([sol[f"VERTEX_SE3__{k}"] for k in range(256)], 1), info.err_history))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])
