"""-m gpu: the fp32 column-pair kernel with its rows regrouped by first non-zero column (thx_hblock_layout.rg_*,
thx_chol_schedule.regroup_rows).  Every row of L keeps its own products in their order and everything left out is a product with
an exact zero, so with regrouping on and off L, the solve panels, y and whole LM trajectories must be the same (torch.equal: -0
and +0 are equal)."""
import numpy as np
import pytest
import torch

from tests.test_gpu_zero_block_skip import GATHER, _factor, _kernels, _random_blocks
from tests.test_row_groups_host import _case

pytestmark = pytest.mark.gpu

# case -> (n, rows of the last group of pair j = 2, first chunks of pair j = 2's groups)
EXPECT = {"p125": (750, 110, [0, 2]), "p128": (768, 128, [0, 3]), "hub125": (750, 110, [0, 8])}


def _topology(name):
    from theseus_amd.utils.synthetic import pose_graph_topology
    if name == "p128":
        return pose_graph_topology(128, 512, 0), 128
    return _case(name)


@pytest.mark.parametrize("gather", list(GATHER))
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("topo", list(EXPECT))
def test_regrouping_rows_leaves_the_factor_unchanged(topo, split, gather):
    edges, P = _topology(topo)
    B = 8
    hb, dhb, Hc, n = _random_blocks(edges, P, B, seed=11)
    rg = hb.row_groups()
    g0, g1 = int(rg.group_ptr[1]), int(rg.group_ptr[2])
    assert (n, int((rg.rows[g1 - 1] >= 0).sum()), rg.k0[g0:g1].tolist()) == EXPECT[topo]
    both = np.diff(rg.tile_ptr).reshape(-1, 2).sum(1)
    if topo == "hub125":   # a K-loop of zero iterations; more pieces than the 42 the registers hold: the overflow path runs
        assert rg.k0[g1 - 1] == 4 * 2 and both.max() > 42
    rhs = torch.randn(B, n, dtype=torch.float32, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    out = []
    for regroup in (1, 0):
        Ks = _kernels(split_diag_min_batch=0 if split else 2 ** 31 - 1, hb_scatter_max_pieces=GATHER[gather],
                      right_looking_max_batch=0, column_pairs_min_batch=0, column_pairs=1, skip_zero_blocks=1, regroup_rows=regroup)
        p = Ks.chol_plan(n, (n + 127) // 128 * 128, B, torch.float32, damping=True, rhs=True, ldv=rhs.stride(0), layout=dhb.c)
        assert p["right_looking"] == 0 and p["column_pairs"] == 1 and p["split_diag"] == int(split), p
        assert p["regroup_rows"] == regroup and rg.k0.max() > 0, p
        out.append(_factor(Ks, dhb, Hc, n, B, rhs))
    (La, Pa, ya), (Lb, Pb, yb) = out
    assert torch.equal(La, Lb) and torch.equal(ya, yb)
    for u in range(4):          # the ten lower sub-blocks of every panel (the others are never written)
        for v in range(u + 1):
            assert torch.equal(Pa[:, :, 32 * u:32 * u + 32, 32 * v:32 * v + 32], Pb[:, :, 32 * u:32 * u + 32, 32 * v:32 * v + 32])
    assert La.abs().sum() > 0 and torch.isfinite(La).all()


def test_regrouping_rows_leaves_the_lm_solution_unchanged():
    """Three LM iterations of the headline graph at 128 problems (the column-pair schedule's default floor) with regrouping on and
    off: the solved poses and the error history are the same."""
    import theseus_amd as th
    from theseus_amd.utils import synthetic as syn
    edges = syn.pose_graph_topology(256, 1024, topology_seed=0)
    res = []
    for regroup in (1, 0):
        obj = syn.build_pose_graph_objective(edges, 256, dtype=torch.float32, device="cuda")
        opt = th.LevenbergMarquardt(obj, linear_solver_cls=th.HipCholeskySolver, max_iterations=3, abs_err_tolerance=0.0,
                                    rel_err_tolerance=0.0, step_size=1.0)
        K = opt.linear_solver.K
        prev = K.chol_schedule.regroup_rows
        K.chol_schedule.regroup_rows = regroup
        try:
            inputs = syn.input_dict(syn.make_pose_graph_tensors(edges, 256, 128, dtype=torch.float32, device="cuda", seed=99))
            sol, info = th.TheseusLayer(opt).forward(inputs, optimizer_kwargs=dict(damping=1e-3, track_err_history=True))
        finally:
            K.chol_schedule.regroup_rows = prev
        res.append((torch.stack([sol[f"VERTEX_SE3__{k}"] for k in range(256)], 1), info.err_history))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])
