"""Host tables of the sorted columns of the fp32 column pairs (thx_hblock_layout.sc_*, theseus_amd/compiler.py:PairColumns): the
256 rows of tiles j, j + 1 sorted by their first non-zero column, cut into eight blocks of 32, a first k-chunk per block and a mask
of active blocks per k-chunk.  No GPU: numpy only, plus the host-only plan query."""
import hashlib

import numpy as np
import pytest

TILE = 128


def _late_closures(P, late, early):
    """The odometry chain of P poses, and every pose >= late tied to one of the first ``early`` poses: the rows below an early pair
    begin at column 0 (its K-loop runs) while the pair's own rows are the chain's (they begin 6 columns left of the diagonal)."""
    return sorted(set([(k - 1, k) for k in range(1, P)] + [(p % early, p) for p in range(late, P)]))


def _graph(name):
    """name -> (edges, poses).  The pairs j >= 2 begin at row 128 j: 256 = 6 * 42 + 4 and 512 = 6 * 85 + 2, so a six-row variable
    straddles both edges of pair j = 2 in every graph here."""
    from theseus_amd.utils.synthetic import pose_graph_topology
    if name == "headline":
        return pose_graph_topology(256, 1024, 0), 256
    if name == "p90":          # n = 540: five tile columns, the last one partial (28 rows below pair j = 2)
        return pose_graph_topology(90, 150, 0), 90
    if name == "p128":         # n = 768: six tile columns
        return pose_graph_topology(128, 400, 0), 128
    if name == "p140":         # n = 840: seven tile columns, pairs j = 0, 2, 4; another seed.  The last twelve poses (the rows below
        # pair j = 4) reach back to poses 18 ... 29 only, so that pair j = 4 is regrouped and sorted as well
        return sorted(set(pose_graph_topology(128, 390, 1) + [(k - 1, k) for k in range(128, 140)] + [(p - 110, p) for p in range(128, 140)])), 140
    if name == "never140":     # pair j = 2's rows are the chain's: seven of its eight blocks begin at or behind its own columns
        return _late_closures(140, 100, 10), 140
    if name == "all0":         # every row of pair j = 2 begins at column 0, the rows from pose 96 on do not: groups, no table
        return sorted(set([(k - 1, k) for k in range(1, 128)] + [(0, p) for p in range(2, 96)])), 128
    raise KeyError(name)


CASES = ["headline", "p90", "p128", "p140", "never140"]
_CACHE = {}


def _tables(name):
    if name not in _CACHE:
        from theseus_amd.compiler import PoseGraphStructure
        edges, P = _graph(name)
        hb = PoseGraphStructure.build(P, edges, [0], dof=6).hessian_blocks()
        _CACHE[name] = (hb, hb.row_groups(), hb.pair_columns())
    return _CACHE[name]


def _symbolic_factor(hb):
    """(n, n) bool: the non-zeros of the natural-order factor, from a numpy symbolic factorisation at variable granularity (column
    k's structure below its first sub-diagonal non-zero p is added to column p)."""
    P = hb.nvars
    S = np.zeros((P, P), bool)
    for a, b in hb.blocks.tolist():
        S[a, b] = True
    for k in range(P):
        below = np.nonzero(S[k + 1:, k])[0] + k + 1
        if below.size > 1:
            S[below[1:], below[0]] = True
    return np.tril(np.kron(S, np.ones((hb.bd, hb.bd), bool)))


@pytest.mark.parametrize("name", CASES)
def test_tables_exist_where_a_block_starts_late_and_only_on_regrouped_pairs(name):
    hb, rg, pc = _tables(name)
    assert rg is not None and pc is not None and pc.npairs == rg.npairs == (hb.ntiles - 1) // 2
    assert pc.has[0] == 0 and pc.has.sum() == pc.npairs_sorted > 0          # pair 0 has no K-loop
    assert pc.has[1] == 1                                                   # every graph here sorts pair j = 2
    assert pc.perm.shape == (pc.npairs, 2 * TILE) and pc.mask.shape == (pc.npairs, 4 * hb.ntiles)
    for jp in range(pc.npairs):
        if not pc.has[jp]:
            assert np.array_equal(pc.perm[jp], np.arange(2 * TILE)) and (pc.mask[jp] == 255).all()
            continue
        assert rg.group_ptr[jp + 1] > rg.group_ptr[jp] and pc.first_chunk[jp].max() > 0


@pytest.mark.parametrize("name", CASES)
def test_permutation_is_a_stable_sort_by_first_column(name):
    hb, rg, pc = _tables(name)
    for jp in np.nonzero(pc.has)[0].tolist():
        perm = pc.perm[jp]
        assert np.array_equal(np.sort(perm), np.arange(2 * TILE))           # a bijection of 0 ... 255
        f = hb.row_first[TILE * 2 * jp + perm].astype(np.int64)
        assert (np.diff(f) >= 0).all()
        same = np.diff(f) == 0
        assert (np.diff(perm)[same] > 0).all()                              # stable ...
        rows = TILE * 2 * jp + perm
        for v in np.unique(rows // hb.bd).tolist():                         # ... so a variable's rows stay adjacent and in order
            s = np.nonzero(rows // hb.bd == v)[0]
            assert np.array_equal(s, np.arange(s[0], s[0] + s.size)) and (np.diff(rows[s]) == 1).all()
        assert np.array_equal(pc.first_chunk[jp], f.reshape(8, 32).min(1) // 32)


@pytest.mark.parametrize("name", CASES)
def test_inactive_blocks_are_zero_in_the_symbolic_factor(name):
    """For every (pair, chunk, block) the mask calls inactive, every entry of the dense symbolic natural-order factor is zero in the
    block's 32 rows and the chunk's 32 columns -- and the mask is exactly kc >= first_chunk."""
    hb, rg, pc = _tables(name)
    Lnz = _symbolic_factor(hb)
    left_out = 0
    for jp in np.nonzero(pc.has)[0].tolist():
        j = 2 * jp
        for kc in range(4 * j):
            m = int(pc.mask[jp, kc])
            assert 0 <= m <= 255
            for u in range(8):
                assert ((m >> u) & 1) == int(kc >= pc.first_chunk[jp, u])
                if not (m >> u) & 1:
                    rows = TILE * j + pc.perm[jp, 32 * u:32 * u + 32]
                    assert not Lnz[rows, 32 * kc:32 * kc + 32].any(), (jp, kc, u)
                    left_out += 1
        assert (pc.mask[jp, 4 * j:] == 255).all()
    assert left_out > 0


def test_a_block_that_never_becomes_active_and_a_pair_without_a_table():
    hb, rg, pc = _tables("never140")
    assert (pc.first_chunk[1] >= 8).sum() == 7 and pc.first_chunk[1, 0] < 8     # pair j = 2: its K-loop is chunks 0 ... 7
    assert int(rg.k0[rg.group_ptr[1]]) == 0                                      # ... and runs from chunk 0 for the late poses' rows
    from theseus_amd.compiler import PoseGraphStructure
    edges, P = _graph("all0")
    hb0 = PoseGraphStructure.build(P, edges, [0], dof=6).hessian_blocks()
    rg0 = hb0.row_groups()
    assert rg0 is not None and rg0.group_ptr[2] > rg0.group_ptr[1]               # pair j = 2 is regrouped
    assert hb0.pair_columns() is None                                           # all eight blocks start at chunk 0: no table
    assert hb0.on("cpu").c.sc_perm is None and hb0.on("cpu").c.sc_pair_host is None


def test_headline_model_matches_the_tables():
    hb, rg, pc = _tables("headline")
    per, (today, srt) = pc.executed_fraction(rg)
    _, skipped = rg.skipped_fraction(hb.l_mask())
    assert abs(today - (1.0 - skipped)) < 1e-12                                  # the project's own count of the regrouped pairs
    assert srt < today - 0.1 and all(b < a for a, b in per.values())
    assert [round(b, 3) for _, b in per.values()] == [0.197, 0.469, 0.674, 0.818]


def _digest(hb, rg):
    h = hashlib.sha256()
    arrays = [hb.blocks, hb.diag_blk, hb.inc_blk, hb.tile_ptr, hb.piece_blk, hb.piece_rc, hb.row_first, hb.l_mask(),
              rg.group_ptr, rg.rows, rg.k0, rg.zf, rg.tile_ptr, rg.piece_blk, rg.piece_rc,
              rg.rows0, rg.zf0, rg.tile_ptr0, rg.piece_blk0, rg.piece_rc0]
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


# sha256 of every table that existed before the sorted columns, taken from the commit before them
OLDER_TABLES = {
    "headline": "9589aa600de400176c5096189319e1560917a862382c98826f9316fc4a53c011",
    "never140": "557cd0ca1029af466e5132bb190af9baf1a364830aa36f6eae0d6b11ffefc791",
}


@pytest.mark.parametrize("name", list(OLDER_TABLES))
def test_older_tables_are_unchanged(name):
    hb, rg, pc = _tables(name)
    assert _digest(hb, rg) == OLDER_TABLES[name]
    # ... and the layout struct has the new fields next to the row groups', in front of row_first, which stays last
    from theseus_amd import _lib
    names = [f for f, _ in _lib.HBlockLayout._fields_]
    assert names[-5:] == ["rg0_max_tile_pieces", "sc_pair_host", "sc_perm", "sc_mask", "row_first"]
    assert [f for f, _ in _lib.CholSchedule._fields_][-2:] == ["skip_zero_solves", "sort_pair_columns"]


def test_plan_reports_sorted_columns_and_their_switches():
    from theseus_amd import _lib
    from theseus_amd.kernels import chol_plan
    import torch
    hb, rg, pc = _tables("headline")
    layout = hb.on("cpu").c      # (the plan reads which tables are set, never their contents)

    def plan(B=4096, dtype=torch.float32, layout=layout, **kw):
        s = _lib.CholSchedule(*([-1] * len(_lib.CholSchedule._fields_)))
        for k, v in kw.items():
            setattr(s, k, v)
        return chol_plan(6 * hb.nvars, hb.ntiles * TILE, B, dtype, layout=layout, schedule=s)
    assert plan()["sort_pair_columns"] == 1 and plan()["regroup_rows"] == 1
    assert plan(sort_pair_columns=0)["sort_pair_columns"] == 0 and plan(sort_pair_columns=0)["regroup_rows"] == 1
    assert plan(regroup_rows=0)["sort_pair_columns"] == 0
    assert plan(skip_zero_blocks=0)["sort_pair_columns"] == 0
    assert plan(skip_zero_solves=0)["sort_pair_columns"] == 1
    assert plan(dtype=torch.float64)["sort_pair_columns"] == 0
    assert plan(B=8)["sort_pair_columns"] == 0                   # (right-looking)
    bare = _lib.HBlockLayout()
    for f, _ in _lib.HBlockLayout._fields_:
        setattr(bare, f, getattr(layout, f))
    bare.sc_mask = None
    assert plan(layout=bare)["sort_pair_columns"] == 0
