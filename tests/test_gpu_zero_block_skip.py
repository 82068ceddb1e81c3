"""-m gpu: the fp32 column-by-column factorisation of a block-compact H skips the K-loop products of structurally zero 32x32
sub-blocks of L (thx_hblock_layout.l_mask, thx_chol_schedule.skip_zero_blocks).  The skipped products are exact zeros, so with
skipping on and off L, the solve panels, y and whole LM trajectories must be the same (torch.equal: -0 and +0 are equal)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GATHER = {"mfma": -1, "lds": 0}


def _kernels(**fields):
    from theseus_amd.kernels import HipKernels
    Ks = HipKernels()
    for k, v in fields.items():
        setattr(Ks.chol_schedule, k, v)
    return Ks


def _random_blocks(edges, P, B, seed):
    """A random SPD H (fp32, diagonally dominant) with exactly the block pattern of ``edges``, as the layout's block list."""
    from theseus_amd.compiler import PoseGraphStructure
    s = PoseGraphStructure.build(P, edges, [0], dof=6)
    hb = s.hessian_blocks()
    n = 6 * P
    rng = np.random.default_rng(seed)
    H = np.zeros((B, n, n))
    for a, b in hb.blocks.tolist():
        H[:, 6 * a:6 * a + 6, 6 * b:6 * b + 6] = rng.standard_normal((B, 6, 6))
    H = np.tril(H, -1)
    H = H + H.transpose(0, 2, 1)
    idx = np.arange(n)
    H[:, idx, idx] = np.abs(H).sum(2) + 1.0 + rng.random((B, n))
    Hc = torch.from_numpy(hb.pack_dense(np.tril(H)).astype(np.float32)).cuda()
    return hb, hb.on("cuda"), Hc, n


def _factor(Ks, dhb, Hc, n, B, rhs):
    nt = (n + 127) // 128
    ld = nt * 128
    lam = torch.full((B,), 1e-3, dtype=torch.float32, device="cuda")
    L = torch.zeros(B, ld, ld, dtype=torch.float32, device="cuda")
    panels = torch.zeros(B, nt, 128, 128, dtype=torch.float32, device="cuda")
    info = torch.empty(B, dtype=torch.int32, device="cuda")
    y = torch.empty_like(rhs)
    Ks.chol_factor_hblocks(dhb, Hc, n, lam, False, 1e-8, L, panels, info, rhs=rhs, y=y)
    assert int(info.abs().sum()) == 0
    return torch.tril(L[:, :n, :n]), panels, y


def _topology(name):
    from theseus_amd.utils.synthetic import chain_graph_topology, pose_graph_topology
    if name == "headline":
        return pose_graph_topology(256, 1024, 0), 256
    if name == "chain_n1500":   # n = 1500: the last tile is partial
        return chain_graph_topology(250), 250
    raise KeyError(name)


@pytest.mark.parametrize("pairs", [True, False])
@pytest.mark.parametrize("gather", list(GATHER))
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("topo", ["headline", "chain_n1500"])
def test_skipping_zero_blocks_leaves_the_factor_unchanged(topo, split, gather, pairs):
    edges, P = _topology(topo)
    B = 8
    hb, dhb, Hc, n = _random_blocks(edges, P, B, seed=7)
    m = hb.l_mask()
    rhs = torch.randn(B, n, dtype=torch.float32, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    out = []
    for skip in (1, 0):
        Ks = _kernels(split_diag_min_batch=0 if split else 2 ** 31 - 1, hb_scatter_max_pieces=GATHER[gather],
                      right_looking_max_batch=0, column_pairs_min_batch=0, column_pairs=int(pairs), skip_zero_blocks=skip)
        p = Ks.chol_plan(n, (n + 127) // 128 * 128, B, torch.float32, damping=True, rhs=True, ldv=rhs.stride(0), layout=dhb.c)
        assert p["right_looking"] == 0 and p["column_pairs"] == int(pairs) and p["split_diag"] == int(split), p
        out.append(_factor(Ks, dhb, Hc, n, B, rhs))
    (La, Pa, ya), (Lb, Pb, yb) = out
    assert torch.equal(La, Lb) and torch.equal(ya, yb)
    for u in range(4):          # the ten lower sub-blocks of every panel (the others are never written)
        for v in range(u + 1):
            assert torch.equal(Pa[:, :, 32 * u:32 * u + 32, 32 * v:32 * v + 32], Pb[:, :, 32 * u:32 * u + 32, 32 * v:32 * v + 32])
    # what the mask calls zero is zero in the factor
    Lz = La.cpu().numpy()
    for t in range(m.shape[0]):
        for c in range(m.shape[1]):
            for s in range(4):
                r0 = 128 * t + 32 * s
                if r0 < n and not (m[t, c] >> s) & 1:
                    assert not Lz[:, r0:r0 + 32, 32 * c:32 * c + 32].any(), (t, c, s)


def test_skipping_zero_blocks_leaves_the_lm_solution_unchanged():
    """Three LM iterations of the headline graph at 128 problems (the column-pair schedule's default floor) with skipping on and
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
        prev = K.chol_schedule.skip_zero_blocks
        K.chol_schedule.skip_zero_blocks = skip
        try:
            inputs = syn.input_dict(syn.make_pose_graph_tensors(edges, 256, 128, dtype=torch.float32, device="cuda", seed=99))
            sol, info = th.TheseusLayer(opt).forward(inputs, optimizer_kwargs=dict(damping=1e-3, track_err_history=True))
        finally:
            K.chol_schedule.skip_zero_blocks = prev
        res.append((torch.stack([sol[f"VERTEX_SE3__{k}"] for k in range(256)], 1), info.err_history))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])
