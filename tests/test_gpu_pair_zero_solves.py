"""-m gpu: the fp32 column-pair kernel with every wave leaving out the solves its strip's first non-zero chunk makes zero, and
pair 0 on row groups of its own (thx_hblock_layout.rg_zf / rg0_*, thx_chol_schedule.skip_zero_solves).  Every output element keeps
its products in their order and everything left out is a product with an exact zero, so with the switch on and off L, the solve
panels, y and whole LM trajectories must be the same (torch.equal: -0 and +0 are equal).  L is filled with NaN before every
factorisation: a zero the kernel should have stored and did not is a NaN, not a stale zero."""
import numpy as np
import pytest
import torch

from tests.test_gpu_zero_block_skip import GATHER, _kernels, _random_blocks
from tests.test_row_groups_host import _case

pytestmark = pytest.mark.gpu

# case -> n
EXPECT = {"p64": 384, "p125": 750, "p128": 768, "hub125": 750, "chain250": 1500}


def _topology(name):
    from theseus_amd.utils.synthetic import pose_graph_topology
    if name == "p64":
        return pose_graph_topology(64, 128, 0), 64
    if name == "p128":
        return pose_graph_topology(128, 512, 0), 128
    return _case(name)


def _factor_nan(Ks, dhb, Hc, n, B, rhs):
    """tests.test_gpu_zero_block_skip._factor with L pre-filled with NaN (the factorisation must write every element of the lower
    triangle it leaves behind, structural zeros included)."""
    nt = (n + 127) // 128
    ld = nt * 128
    lam = torch.full((B,), 1e-3, dtype=torch.float32, device="cuda")
    L = torch.full((B, ld, ld), float("nan"), dtype=torch.float32, device="cuda")
    panels = torch.zeros(B, nt, 128, 128, dtype=torch.float32, device="cuda")
    info = torch.empty(B, dtype=torch.int32, device="cuda")
    y = torch.empty_like(rhs)
    Ks.chol_factor_hblocks(dhb, Hc, n, lam, False, 1e-8, L, panels, info, rhs=rhs, y=y)
    assert int(info.abs().sum()) == 0
    return torch.tril(L[:, :n, :n]), panels, y


def _run(topo, split, gather, B):
    edges, P = _topology(topo)
    hb, dhb, Hc, n = _random_blocks(edges, P, B, seed=11)
    rg = hb.row_groups()
    assert n == EXPECT[topo] and rg.ngroups0 > 0
    z0 = np.clip(rg.zf0, 0, 8)
    if topo == "p64":       # the four wave states in one workgroup: no skip, partial X0, X0 = 0, X0 = 0 and a partial X1
        assert rg.ngroups == 0 and z0.tolist() == [[0, 2, 4, 7]]
    if topo == "hub125":    # a K-loop of zero iterations next to z > 0; more pieces than the 42 the registers hold
        g0, g1 = int(rg.group_ptr[1]), int(rg.group_ptr[2])
        assert rg.k0[g1 - 1] == 8 and (rg.zf[g1 - 1] >= 8).all() and np.diff(rg.tile_ptr).reshape(-1, 2).sum(1).max() > 42
    if topo == "chain250":  # groups that lie wholly behind their pair, in every pair: they only store zeros
        for jp in range(rg.npairs):
            zf = rg.zf0 if jp == 0 else rg.zf[int(rg.group_ptr[jp]):int(rg.group_ptr[jp + 1])]
            assert (zf.min(1) >= 8 * jp + 8).any(), jp
    rhs = torch.randn(B, n, dtype=torch.float32, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    out = []
    for skip in (1, 0):
        Ks = _kernels(split_diag_min_batch=0 if split else 2 ** 31 - 1, hb_scatter_max_pieces=GATHER[gather], right_looking_max_batch=0,
                      column_pairs_min_batch=0, column_pairs=1, skip_zero_blocks=1, regroup_rows=1, skip_zero_solves=skip)
        p = Ks.chol_plan(n, (n + 127) // 128 * 128, B, torch.float32, damping=True, rhs=True, ldv=rhs.stride(0), layout=dhb.c)
        assert p["right_looking"] == 0 and p["column_pairs"] == 1 and p["split_diag"] == int(split), p
        assert p["skip_zero_solves"] == skip and p["regroup_rows"] == int(rg.ngroups > 0), p
        out.append(_factor_nan(Ks, dhb, Hc, n, B, rhs))
    (La, Pa, ya), (Lb, Pb, yb) = out
    assert torch.isfinite(La).all() and torch.isfinite(Lb).all() and La.abs().sum() > 0
    assert torch.equal(La, Lb) and torch.equal(ya, yb)
    for u in range(4):          # the ten lower sub-blocks of every panel (the others are never written)
        for v in range(u + 1):
            assert torch.equal(Pa[:, :, 32 * u:32 * u + 32, 32 * v:32 * v + 32], Pb[:, :, 32 * u:32 * u + 32, 32 * v:32 * v + 32])


@pytest.mark.parametrize("gather", list(GATHER))
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("topo", list(EXPECT))
def test_skipping_zero_solves_leaves_the_factor_unchanged(topo, split, gather):
    _run(topo, split, gather, 8)


def test_skipping_zero_solves_with_a_batch_that_is_no_multiple_of_eight():
    _run("p125", False, list(GATHER)[0], 5)


def test_skipping_zero_solves_leaves_the_lm_solution_unchanged():
    """Three LM iterations of the headline graph at 128 problems (the column-pair schedule's default floor) with the switch on and
    off: the solved poses and the error history are the same."""
    import theseus_amd as th
    from theseus_amd.utils import synthetic as syn
    edges = syn.pose_graph_topology(256, 1024, topology_seed=0)
    res = []
    for skip in (1, 0):
        obj = syn.build_pose_graph_objective(edges, 256, dtype=torch.float32, device="cuda")
        opt = th.LevenbergMarquardt(obj, linear_solver_cls=th.HipCholeskySolver, max_iterations=3, abs_err_tolerance=0.0,
                                    rel_err_tolerance=0.0, step_size=1.0)
        K = opt.linear_solver.K
        prev = K.chol_schedule.skip_zero_solves
        K.chol_schedule.skip_zero_solves = skip
        try:
            inputs = syn.input_dict(syn.make_pose_graph_tensors(edges, 256, 128, dtype=torch.float32, device="cuda", seed=99))
            sol, info = th.TheseusLayer(opt).forward(inputs, optimizer_kwargs=dict(damping=1e-3, track_err_history=True))
        finally:
            K.chol_schedule.skip_zero_solves = prev
        res.append((torch.stack([sol[f"VERTEX_SE3__{k}"] for k in range(256)], 1), info.err_history))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])
