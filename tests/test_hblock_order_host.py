"""CPU side of the dense solver's own variable order (thx_hblock_order, theseus_amd/compiler.py:OrderedHessianBlocks): the order is a
deterministic permutation that never scores above the insertion order and leaves a chain alone; the layout built on it is the
layout of P H P^T -- its tables against a dense symbolic factor of the permuted pattern, as tests/test_solve_envelope_host.py
checks the natural one -- and the block map moves every block of the linearization's list to its place, transposed where its two
variables swap sides of the diagonal."""
import numpy as np
import pytest

from tests.test_solve_envelope_host import layout, symbolic_factor

GRAPHS = ["p48", "p70", "path70", "star48", "headline"]


def order(hb):
    from theseus_amd import _lib
    return _lib.hblock_order(hb.blocks, hb.nvars, hb.bd)


def envelope_score(hb, perm):
    """sum over scalar rows of (r - first[r])^2 of P H P^T, from the block pattern alone."""
    d, P = hb.bd, hb.nvars
    pos = np.empty(P, dtype=np.int64)
    pos[perm] = np.arange(P)
    first = np.arange(P)
    a, b = pos[hb.blocks[:, 0]], pos[hb.blocks[:, 1]]
    np.minimum.at(first, np.maximum(a, b), np.minimum(a, b))
    w = d * (np.arange(P) - first)
    return int(sum(((w + i) ** 2).sum() for i in range(d)))


@pytest.mark.parametrize("name", GRAPHS)
def test_order_is_a_deterministic_permutation_that_never_scores_above_insertion_order(name):
    hb = layout(name)
    perm, score, natural = order(hb)
    assert perm.dtype == np.int32 and np.array_equal(np.sort(perm), np.arange(hb.nvars))
    assert score <= natural
    assert score == envelope_score(hb, perm) and natural == envelope_score(hb, np.arange(hb.nvars))
    again = order(hb)
    assert np.array_equal(again[0], perm) and again[1:] == (score, natural)
    if score == natural:
        assert np.array_equal(perm, np.arange(hb.nvars))   # a tie keeps the insertion order


def test_a_chain_comes_back_as_the_identity_and_a_star_moves_its_hub_to_the_end():
    from theseus_amd.compiler import ordered_hessian_blocks
    hb = layout("path70")
    perm, score, natural = order(hb)
    assert np.array_equal(perm, np.arange(hb.nvars)) and score == natural
    assert ordered_hessian_blocks(hb) is None
    # a star around variable 0: with the hub in front every row begins at column 0; behind its leaves only the hub's own row is long
    hb = layout("star48")
    perm, score, natural = order(hb)
    assert score < natural and 0 in perm[-2:].tolist()
    oh = ordered_hessian_blocks(hb)
    assert oh.nswapped >= hb.nvars - 2                      # every spoke but one lands transposed


def test_the_headline_envelope_shrinks_as_modelled():
    """The symbolic model the order was chosen by: envelope non-zeros of tril(L) 0.72 -> below 0.55, sum (row length)^2 below
    0.6 of the insertion order's."""
    hb = layout("headline")
    perm, score, natural = order(hb)
    assert score < 0.6 * natural
    from theseus_amd.compiler import ordered_hessian_blocks
    oh = ordered_hessian_blocks(hb)
    n = hb.bd * hb.nvars
    share = lambda first: float((np.arange(n) - first + 1).sum()) / (n * (n + 1) / 2)   # noqa: E731
    assert 0.71 < share(hb.row_first) < 0.73 and share(oh.layout.row_first) < 0.55


def test_bad_arguments_are_refused():
    from theseus_amd import _lib
    lib = _lib.load()
    blocks = np.array([[0, 0], [1, 0], [1, 1]], dtype=np.int32)
    perm = np.zeros(2, dtype=np.int32)
    assert lib.thx_hblock_order(2, 6, 3, blocks.ctypes.data, None, None) != 0
    assert lib.thx_hblock_order(0, 6, 3, blocks.ctypes.data, perm.ctypes.data, None) != 0
    upper = np.array([[0, 1]], dtype=np.int32)
    assert lib.thx_hblock_order(2, 6, 1, upper.ctypes.data, perm.ctypes.data, None) != 0
    assert b"outside tril" in lib.thx_last_error()
    assert lib.thx_hblock_order(2, 6, 3, blocks.ctypes.data, perm.ctypes.data, None) == 0   # (no score asked for)
    assert perm.tolist() == [0, 1]
    for name in ("thx_hblock_order", "thx_hblocks_permute"):
        assert name in _lib.EXPORTED_SYMBOLS


@pytest.mark.parametrize("name", ["p48", "p70", "headline"])
def test_tables_of_the_permuted_layout_agree_with_a_symbolic_factor_of_the_permuted_matrix(name):
    from theseus_amd.compiler import ordered_hessian_blocks
    hb = layout(name)
    oh = ordered_hessian_blocks(hb)
    assert oh is not None and oh.nswapped > 0          # at least one block lands transposed
    lay, d, P = oh.layout, hb.bd, hb.nvars
    n = d * P
    # the permuted layout's pattern is the natural one's under pos: the same blocks, each once
    want = {(max(oh.pos[a], oh.pos[b]), min(oh.pos[a], oh.pos[b])) for a, b in hb.blocks.tolist()}
    assert {tuple(x) for x in lay.blocks.tolist()} == want and lay.nblocks == hb.nblocks == len(want)
    # row_first against the dense symbolic factor of P H P^T (tests/test_solve_envelope_host.py, same check)
    S = symbolic_factor(lay)
    first, cols = lay.row_first, np.arange(n)
    for r in range(n):
        nz = cols[S[r]]
        assert nz[0] >= first[r] and nz[0] // d == first[r] // d, r
    # l_mask marks every 32 x 32 sub-block the factor touches
    m, nt = lay.l_mask(), lay.ntiles
    pad = np.zeros((128 * nt, 128 * nt), bool)
    pad[:n, :n] = S
    sub = pad.reshape(4 * nt, 32, 4 * nt, 32).any(axis=(1, 3))
    for R in range(4 * nt):
        for C in range(R + 1):
            if sub[R, C]:
                assert (m[R // 4, C] >> (R % 4)) & 1, (R, C)
    # the row groups, sorted columns and sorted rows are built on the permuted first
    rg = lay.row_groups()
    if rg is not None:
        assert np.array_equal(rg.first, lay.row_first)


@pytest.mark.parametrize("name", ["p48", "headline"])
def test_block_map_moves_every_block_to_its_place_and_transposes_the_swapped_ones(name):
    from theseus_amd.compiler import ordered_hessian_blocks
    hb = layout(name)
    oh = ordered_hessian_blocks(hb)
    d, n = hb.bd, hb.bd * hb.nvars
    rng = np.random.default_rng(3)
    H = np.tril(rng.standard_normal((1, n, n)))
    Hc = hb.pack_dense(H)                                   # the linearization's list: blocks of tril(H) in its own order
    src, t = oh.block_map >> 1, oh.block_map & 1
    assert np.array_equal(np.sort(src), np.arange(hb.nblocks)) and int(t.sum()) == oh.nswapped
    blocks = Hc[:, :hb.elems].reshape(1, hb.nblocks, d, d)
    moved = np.where(t[None, :, None, None] == 1, blocks[:, src].transpose(0, 1, 3, 2), blocks[:, src])
    Hp = np.zeros((1, oh.layout.bstride))
    Hp[:, :oh.layout.elems] = moved.reshape(1, -1)
    # ... expanded through the permuted layout's pieces it is P H P^T (lower triangle; diagonal blocks in full, as the list has them)
    full = np.tril(H[0], -1) + np.tril(H[0], -1).T
    for v in range(hb.nvars):
        full[d * v:d * v + d, d * v:d * v + d] = H[0, d * v:d * v + d, d * v:d * v + d]
    want = full[np.ix_(oh.to_perm, oh.to_perm)]
    got = oh.layout.expand(Hp, n)[0]
    mask = np.zeros((n, n), bool)                            # (what the tiles read: blocks on and below the block diagonal)
    for a, b in oh.layout.blocks.tolist():
        mask[d * a:d * a + d, d * b:d * b + d] = True
    assert np.array_equal(got[mask], want[mask]) and not got[~mask].any()
    # the vector maps are each other's inverse and follow the variables
    assert np.array_equal(oh.to_perm[oh.from_perm], np.arange(n))
    assert np.array_equal(oh.to_perm.reshape(-1, d)[:, 0] // d, oh.perm)
