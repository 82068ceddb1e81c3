"""-m gpu: the fp32 SYRK of the split diagonal phase and the column pairs' head tiles with a tile's 128 rows staged in ascending order
of their first non-zero column (thx_hblock_layout.tr_* / th_*, thx_chol_schedule.sort_tile_rows).  Every output element keeps its products in their order, what is
left out is a product with an exact zero, and the accumulators return to natural order before anything else reads them: with the
switch on and off L, the solve panels, y and the solution must be the same (torch.equal: -0 and +0 are equal).  L is filled with NaN
before every factorisation: an element the kernel should have stored and did not is a NaN, not a stale value."""
import pytest
import torch

from tests.test_gpu_pair_sorted_columns import EXPECT, _factor_solve
from tests.test_gpu_zero_block_skip import GATHER, _kernels, _random_blocks
from tests.test_pair_columns_host import _graph
from tests.test_tile_rows_host import _star

pytestmark = pytest.mark.gpu

NEVER_SPLIT = 2 ** 31 - 1


def _case(topo):
    if topo == "star":          # every row begins at column 0: no row groups, no tables -- the switch changes no launch
        return _star(128), 128, (768, 6)
    edges, P = _graph(topo)
    return edges, P, EXPECT[topo]


def _run(topo, split_min, gather, B, sort_cols=1):
    edges, P, expect = _case(topo)
    hb, dhb, Hc, n = _random_blocks(edges, P, B, seed=23)
    tr = hb.tile_rows()
    assert (n, hb.ntiles) == expect
    if topo == "star":
        assert tr is None and hb.row_groups() is None
    else:
        assert tr is not None and tr.has[0] == 0 and tr.has[1:].sum() >= 2 and tr.has32.sum() >= 1   # SYRK tables and a head-tile table
    if topo == "p90":           # the last tile has 28 rows inside the matrix: its padded rows fill block rows that never run
        assert tr.has[4] == 1 and (tr.first_chunk[4] >= 16).sum() >= 6
    if topo == "never140":      # tiles 1 .. 3: seven of the eight blocks begin in the tile's own columns, never active in its K-loop
        assert all((tr.first_chunk[j] >= 4 * j).sum() == 7 for j in (1, 2, 3))
        assert tr.has32[2] == 1 and tr.k0h[2] == 8       # ... and head tile (3, 2) has no chunk to run
    split = B >= split_min
    rhs = torch.randn(B, n, dtype=torch.float32, device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    out = []
    for sort in (1, 0):
        Ks = _kernels(split_diag_min_batch=split_min, hb_scatter_max_pieces=GATHER[gather], right_looking_max_batch=0,
                      column_pairs_min_batch=0, column_pairs=1, skip_zero_blocks=1, regroup_rows=1, sort_pair_columns=sort_cols,
                      sort_tile_rows=sort)
        p = Ks.chol_plan(n, (n + 127) // 128 * 128, B, torch.float32, damping=True, rhs=True, ldv=rhs.stride(0), layout=dhb.c)
        assert p["right_looking"] == 0 and p["column_pairs"] == 1 and p["split_diag"] == int(split), p
        assert p["regroup_rows"] == (0 if topo == "star" else 1), p
        assert p["sort_tile_rows"] == (sort if tr is not None else 0), p          # (never split: the head tiles alone)
        out.append(_factor_solve(Ks, dhb, Hc, n, B, rhs, dhb.t["row_first"]))
    (La, Pa, ya, xa), (Lb, Pb, yb, xb) = out
    assert torch.isfinite(La).all() and torch.isfinite(Lb).all() and La.abs().sum() > 0 and torch.isfinite(xa).all()
    assert torch.equal(La, Lb) and torch.equal(ya, yb) and torch.equal(xa, xb)
    for u in range(4):          # the ten lower sub-blocks of every panel (the others are never written)
        for v in range(u + 1):
            assert torch.equal(Pa[:, :, 32 * u:32 * u + 32, 32 * v:32 * v + 32], Pb[:, :, 32 * u:32 * u + 32, 32 * v:32 * v + 32])


@pytest.mark.parametrize("gather", list(GATHER))
@pytest.mark.parametrize("topo", ["p90", "p128", "p140", "never140", "all0", "star"])
def test_sorting_the_tile_rows_leaves_the_factor_unchanged(topo, gather):
    _run(topo, 0, gather, 8)


@pytest.mark.parametrize("sort_cols", [0, 1])
@pytest.mark.parametrize("topo", ["p90", "p140"])
def test_sorted_tile_rows_with_a_batch_that_is_no_multiple_of_eight(topo, sort_cols):
    _run(topo, 0, list(GATHER)[0], 11, sort_cols=sort_cols)


@pytest.mark.parametrize("sort_cols", [0, 1])
def test_sorted_tile_rows_and_the_pair_columns_switch(sort_cols):
    _run("never140", 0, list(GATHER)[1], 8, sort_cols=sort_cols)


@pytest.mark.parametrize("gather", list(GATHER))
@pytest.mark.parametrize("topo,B", [("p128", 8), ("p140", 11), ("never140", 8)])
def test_the_head_tiles_alone_under_a_fused_diagonal_phase(topo, B, gather):
    _run(topo, NEVER_SPLIT, gather, B)


def test_sorting_the_tile_rows_leaves_the_lm_solution_unchanged():
    """Three LM iterations of the headline graph at 128 problems, the diagonal phase split, with the switch on and off: the solved
    poses and the error history are the same."""
    import theseus_amd as th
    from theseus_amd.utils import synthetic as syn
    edges = syn.pose_graph_topology(256, 1024, topology_seed=0)
    from theseus_amd.compiler import PoseGraphStructure
    layout = PoseGraphStructure.build(256, edges, [0], dof=6).hessian_blocks().on("cpu").c   # (the plan reads which tables are set)
    res = []
    for sort in (1, 0):
        obj = syn.build_pose_graph_objective(edges, 256, dtype=torch.float32, device="cuda")
        opt = th.LevenbergMarquardt(obj, linear_solver_cls=th.HipCholeskySolver, max_iterations=3, abs_err_tolerance=0.0,
                                    rel_err_tolerance=0.0, step_size=1.0)
        K = opt.linear_solver.K
        prev = K.chol_schedule.sort_tile_rows, K.chol_schedule.split_diag_min_batch
        K.chol_schedule.sort_tile_rows, K.chol_schedule.split_diag_min_batch = sort, 0
        p = K.chol_plan(1536, 1536, 128, torch.float32, damping=True, rhs=True, ldv=1536, layout=layout)
        assert p["column_pairs"] == 1 and p["regroup_rows"] == 1 and p["split_diag"] == 1 and p["sort_tile_rows"] == sort, p
        try:
            inputs = syn.input_dict(syn.make_pose_graph_tensors(edges, 256, 128, dtype=torch.float32, device="cuda", seed=99))
            sol, info = th.TheseusLayer(opt).forward(inputs, optimizer_kwargs=dict(damping=1e-3, track_err_history=True))
        finally:
            K.chol_schedule.sort_tile_rows, K.chol_schedule.split_diag_min_batch = prev
        res.append((torch.stack([sol[f"VERTEX_SE3__{k}"] for k in range(256)], 1), info.err_history))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])
