"""Host only: thx_hblock_fill_mask (thx_hblock_layout.l_mask) -- the structurally non-zero 32x32 sub-blocks of the natural-order
Cholesky factor of a block-compact H -- against an independent dense symbolic factorisation and against the zeros of a real
(numpy, fp64) Cholesky factor of a random SPD matrix with the same block pattern."""
import numpy as np
import pytest

from theseus_amd import _lib


def _structure(P, edges):
    from theseus_amd.compiler import PoseGraphStructure
    return PoseGraphStructure.build(P, edges, [0], dof=6).hessian_blocks()


def _topology(name):
    from theseus_amd.utils.synthetic import chain_graph_topology, pose_graph_topology
    if name == "headline":
        return 256, pose_graph_topology(256, 1024, 0)
    if name == "chain":
        return 256, chain_graph_topology(256, shuffle=False)
    if name == "chain_n1500":
        return 250, chain_graph_topology(250)
    raise KeyError(name)


def _sub_blocks(mask):
    """(ntiles, 4 ntiles) 4-bit table -> (4 ntiles, 4 ntiles) bool matrix of 32x32 sub-blocks (row, column)."""
    nt = mask.shape[0]
    bits = (mask[:, None, :] >> np.arange(4)[None, :, None]) & 1       # (tile, s, chunk)
    return bits.reshape(4 * nt, 4 * nt).astype(bool)


def _python_symbolic(blocks, P, bd, nsub):
    """Independent reference: dense boolean elimination at variable granularity, then every variable block of the fill marks the
    32x32 sub-blocks it overlaps (lower triangle)."""
    S = np.zeros((P, P), bool)
    S[blocks[:, 0], blocks[:, 1]] = True
    S |= S.T
    np.fill_diagonal(S, True)
    for k in range(P):
        rows = np.nonzero(S[k + 1:, k])[0] + k + 1
        S[np.ix_(rows, rows)] = True
    out = np.zeros((nsub, nsub), bool)
    for p, q in zip(*np.nonzero(np.tril(S))):
        for R in range(bd * p // 32, (bd * p + bd - 1) // 32 + 1):
            for C in range(bd * q // 32, min((bd * q + bd - 1) // 32, R) + 1):
                out[R, C] = True
    return out


def _kept_fraction(M):
    """Share of the 32x32 block products L_RK L_CK^T (K < C <= R) of the Cholesky updates with both operands non-zero."""
    tot = kept = 0
    for K in range(M.shape[0]):
        col = M[:, K]
        for C in range(K + 1, M.shape[0]):
            tot += M.shape[0] - C
            kept += int((col[C:] & col[C]).sum())
    return kept / tot


@pytest.mark.parametrize("name", ["headline", "chain", "chain_n1500"])
def test_mask_matches_an_independent_symbolic_factorisation(name):
    P, edges = _topology(name)
    hb = _structure(P, edges)
    M = _sub_blocks(hb.l_mask())
    ref = _python_symbolic(np.asarray(hb.blocks), P, 6, M.shape[0])
    np.testing.assert_array_equal(M, ref)
    n = 6 * P
    inside = (np.arange(M.shape[0]) * 32 < n)
    assert not M[~inside].any()                                     # sub-blocks wholly outside the matrix
    assert M[np.arange(M.shape[0])[inside], np.arange(M.shape[0])[inside]].all()   # the diagonal
    if name == "headline":
        # the issue's figures: 1127 of 1176 lower sub-blocks non-zero, ~90 % of the update block products kept
        assert int(np.tril(M).sum()) == 1127 and M.shape[0] * (M.shape[0] + 1) // 2 == 1176
        assert 0.88 < _kept_fraction(M) < 0.91


@pytest.mark.parametrize("name", ["headline", "chain_n1500"])
def test_mask_zeros_are_zeros_of_a_numeric_factor(name):
    P, edges = _topology(name)
    hb = _structure(P, edges)
    M = _sub_blocks(hb.l_mask())
    n = 6 * P
    rng = np.random.default_rng(5)
    H = np.zeros((n, n))
    for a, b in np.asarray(hb.blocks).tolist():
        H[6 * a:6 * a + 6, 6 * b:6 * b + 6] = rng.standard_normal((6, 6))
    H = np.tril(H, -1)
    H = H + H.T
    H[np.arange(n), np.arange(n)] = np.abs(H).sum(1) + 1.0
    L = np.linalg.cholesky(H)
    nsub = (n + 31) // 32
    numeric = np.zeros((M.shape[0], M.shape[0]), bool)
    for R in range(nsub):
        for C in range(R + 1):
            numeric[R, C] = bool(np.any(L[32 * R:32 * R + 32, 32 * C:32 * C + 32] != 0))
    assert not (numeric & ~M).any()          # never a zero where the factor has a non-zero
    np.testing.assert_array_equal(numeric, M)   # (random values: no numeric cancellation either)


def test_dense_pattern_gives_an_all_ones_mask():
    P = 40                                     # n = 240: two tiles, the second one partial
    blocks = np.array([(p, q) for p in range(P) for q in range(p + 1)], np.int32)
    M = _sub_blocks(_lib.hblock_fill_mask(blocks, P, 6))
    inside = np.arange(M.shape[0]) * 32 < 6 * P
    lower = np.tril(np.ones_like(M))
    np.testing.assert_array_equal(M, lower & inside[:, None] & inside[None, :])


def test_bad_block_lists_are_refused():
    with pytest.raises(RuntimeError):
        _lib.hblock_fill_mask(np.array([[0, 1]], np.int32), 4, 6)      # above the diagonal
    with pytest.raises(RuntimeError):
        _lib.hblock_fill_mask(np.array([[9, 0]], np.int32), 4, 6)      # outside the matrix
