"""Host tables of the sorted rows of the diagonal tiles (thx_hblock_layout.tr_*, theseus_amd/compiler.py:TileRows): the 128 rows of
tile j sorted by their first non-zero column, cut into eight rank blocks of 16 that are placed on the SYRK kernel's block rows, a
first k-chunk per block row and a mask of active block rows per k-chunk.  No GPU: numpy only, plus the host-only plan query."""
import numpy as np
import pytest

from tests.test_pair_columns_host import OLDER_TABLES, _digest, _graph, _symbolic_factor, _tables

TILE = 128
CASES = ["headline", "p90", "p128", "p140", "never140", "all0"]
_CACHE = {}


def _star(P):
    """The odometry chain of P poses with every pose tied to pose 0: every row begins at column 0."""
    return sorted(set([(k - 1, k) for k in range(1, P)] + [(0, p) for p in range(2, P)]))


def _tr(name):
    if name not in _CACHE:
        from theseus_amd.compiler import PoseGraphStructure
        edges, P = _graph(name)
        hb = PoseGraphStructure.build(P, edges, [0], dof=6).hessian_blocks()
        _CACHE[name] = (hb, hb.tile_rows())
    return _CACHE[name]


@pytest.mark.parametrize("name", CASES)
def test_every_permutation_is_a_stable_sort_placed_on_the_block_rows(name):
    from theseus_amd.compiler import TileRows
    hb, tr = _tr(name)
    n, nt = hb.bd * hb.nvars, hb.ntiles
    assert tr is not None and tr.has[0] == 0 and tr.has.sum() > 0 and tr.has.sum() + tr.has32.sum() == tr.ntables
    assert tr.perm.shape == (nt, TILE) and tr.mask.shape == (nt, 4 * nt) and tr.first_chunk.shape == (nt, 8)
    assert sorted(TileRows.PLACE) == list(range(8)) and tr.place == TileRows.PLACE
    for j in range(nt):
        if not tr.has[j]:
            assert np.array_equal(tr.perm[j], np.arange(TILE)) and (tr.mask[j] == 255).all()
            continue
        perm = tr.perm[j]
        assert np.array_equal(np.sort(perm), np.arange(TILE))                   # a bijection of 0 ... 127
        ranked = np.concatenate([perm[16 * u:16 * u + 16] for u in TileRows.PLACE])   # rank block q lies at block row PLACE[q]
        rows = TILE * j + ranked
        inside = rows < n
        assert not inside[int(inside.sum()):].any()                             # rows at or behind n go last
        f = hb.row_first[rows[inside]].astype(np.int64)
        assert (np.diff(f) >= 0).all()
        assert (np.diff(rows[inside])[np.diff(f) == 0] > 0).all()               # stable ...
        assert (np.diff(rows[~inside]) > 0).all()
        for v in np.unique(rows[inside] // hb.bd).tolist():                     # ... so a variable's rows stay adjacent and in order
            s = np.nonzero(rows // hb.bd == v)[0]
            assert np.array_equal(s, np.arange(s[0], s[0] + s.size)) and (np.diff(rows[s]) == 1).all()
        for u in range(8):
            blk = TILE * j + perm[16 * u:16 * u + 16]
            blk = blk[blk < n]
            want = int(hb.row_first[blk].min()) // 32 if blk.size else 4 * nt
            assert tr.first_chunk[j, u] == min(want, 4 * nt)
        assert tr.first_chunk[j].max() > 0


@pytest.mark.parametrize("name", CASES)
def test_inactive_block_rows_are_zero_in_the_symbolic_factor(name):
    """For every (tile, chunk, block row) the mask calls inactive, every entry of the dense symbolic natural-order factor is zero
    in the block's rows and the chunk's 32 columns; the masks are exactly kc >= first_chunk, hence monotone in kc; rows at or
    behind n are never active."""
    hb, tr = _tr(name)
    n, nt = hb.bd * hb.nvars, hb.ntiles
    Lnz = np.zeros((nt * TILE, nt * TILE), bool)
    Lnz[:n, :n] = _symbolic_factor(hb)
    left_out = 0
    for j in np.nonzero(tr.has)[0].tolist():
        prev = 0
        for kc in range(4 * j):
            m = int(tr.mask[j, kc])
            assert 0 <= m <= 255 and (m & prev) == prev                          # monotone: an active block row stays active
            prev = m
            for u in range(8):
                assert ((m >> u) & 1) == int(kc >= tr.first_chunk[j, u])
                rows = TILE * j + tr.perm[j, 16 * u:16 * u + 16]
                if not (m >> u) & 1:
                    assert not Lnz[rows, 32 * kc:32 * kc + 32].any(), (j, kc, u)
                    left_out += 1
                elif (rows >= n).all():
                    raise AssertionError(("a block row of padded rows is active", j, kc, u))
        assert (tr.mask[j, 4 * j:] == 255).all()
    assert left_out > 0


@pytest.mark.parametrize("name", CASES)
def test_head_tile_tables(name):
    """Head tile (j + 1, j), j even: perm32 is the plain stable sort of tile j's rows in four blocks of 32, the masks are exactly
    kc >= first_chunk32 (monotone), an inactive block is zero in the symbolic factor at that chunk, and no product of a row of tile
    j + 1 with a row of tile j is structurally non-zero before chunk k0h."""
    hb, tr = _tr(name)
    n, nt = hb.bd * hb.nvars, hb.ntiles
    Lnz = np.zeros((nt * TILE, nt * TILE), bool)
    Lnz[:n, :n] = _symbolic_factor(hb)
    assert tr.perm32.shape == (nt, TILE) and tr.mask32.shape == (nt, 4 * nt) and tr.k0h.shape == (nt,)
    assert tr.has32.sum() > 0 and all(j % 2 == 0 and 2 <= j < nt - 1 for j in np.nonzero(tr.has32)[0].tolist())
    for j in range(nt):
        if not tr.has32[j]:
            assert np.array_equal(tr.perm32[j], np.arange(TILE)) and (tr.mask32[j] == 15).all() and tr.k0h[j] == 0
            continue
        perm = tr.perm32[j]
        assert np.array_equal(np.sort(perm), np.arange(TILE))
        rows = TILE * j + perm
        f = hb.row_first[rows].astype(np.int64)
        assert (np.diff(f) >= 0).all() and (np.diff(perm)[np.diff(f) == 0] > 0).all()          # the plain stable sort
        for v in np.unique(rows // hb.bd).tolist():                                              # a variable's rows adjacent and in order
            s = np.nonzero(rows // hb.bd == v)[0]
            assert np.array_equal(s, np.arange(s[0], s[0] + s.size)) and (np.diff(rows[s]) == 1).all()
        assert np.array_equal(tr.first_chunk32[j], f.reshape(4, 32).min(1) // 32)
        assert tr.first_chunk32[j].max() > 0 or tr.k0h[j] > 0
        prev = 0
        for kc in range(4 * j):
            m = int(tr.mask32[j, kc])
            assert 0 <= m <= 15 and (m & prev) == prev
            prev = m
            for u in range(4):
                assert ((m >> u) & 1) == int(kc >= tr.first_chunk32[j, u])
                if not (m >> u) & 1:
                    assert not Lnz[rows[32 * u:32 * u + 32], 32 * kc:32 * kc + 32].any(), (j, kc, u)
        assert (tr.mask32[j, 4 * j:] == 15).all()
        # the first chunk with a structurally non-zero product L[r, k] L[c, k], r in tile j + 1, c in tile j
        both = Lnz[TILE * (j + 1):TILE * (j + 2), :TILE * j].any(0) & Lnz[TILE * j:TILE * (j + 1), :TILE * j].any(0)
        first_product = int(np.argmax(both)) // 32 if both.any() else 4 * j
        assert 0 <= tr.k0h[j] <= min(first_product, 4 * j), (j, tr.k0h[j], first_product)


def test_head_tile_model_and_a_head_tile_without_a_k_loop():
    hb, tr = _tr("headline")
    per, executed = tr.head_model()
    assert round(executed, 3) == 0.819 and list(per) == [2, 4, 6, 8, 10]
    hb, tr = _tr("never140")          # every row of tile 2 begins in the tile's own columns: its head tile's K-loop has no chunk
    assert tr.has32[2] == 1 and tr.k0h[2] == 8 and (tr.first_chunk32[2] < 8).sum() == 1
    hb, tr = _tr("all0")              # tile 2: all four blocks and tile 3 begin at chunk 0 -- no table
    assert tr.has32.tolist() == [0, 0, 0, 0, 1, 0]


def test_padded_rows_are_never_active():
    for name, n in (("p90", 540), ("p140", 840)):
        hb, tr = _tr(name)
        j = hb.ntiles - 1
        assert hb.bd * hb.nvars == n and n % TILE and tr.has[j] == 1
        padded = [u for u in range(8) if (TILE * j + tr.perm[j, 16 * u:16 * u + 16] >= n).all()]
        assert padded and all(tr.first_chunk[j, u] >= 4 * hb.ntiles for u in padded)
        assert all(not (int(tr.mask[j, kc]) >> u) & 1 for u in padded for kc in range(4 * j))


def test_a_block_that_never_becomes_active_and_layouts_without_tables():
    hb, tr = _tr("never140")
    assert all((tr.first_chunk[j] >= 4 * j).sum() == 7 for j in (1, 2, 3))       # their first lies in the tile's own columns
    hb, tr = _tr("all0")                                                         # tiles whose blocks all begin at chunk 0: no table
    assert tr.has.tolist() == [0, 0, 0, 0, 1, 1]
    from theseus_amd.compiler import PoseGraphStructure
    hb0 = PoseGraphStructure.build(128, _star(128), [0], dof=6).hessian_blocks()   # a layout without late rows
    assert hb0.row_groups() is None and hb0.tile_rows() is None
    c = hb0.on("cpu").c
    assert c.tr_perm16 is None and c.tr_mask16 is None and c.tr_tile_host is None
    assert c.th_perm32 is None and c.th_mask32 is None and c.th_k0h is None and c.th_tile_host is None


def test_headline_model():
    """Executed 16x16 block products and the busiest wave per chunk, as shares of dense: the placement against the identity."""
    from theseus_amd.compiler import TileRows
    hb, tr = _tr("headline")
    per, (executed, slowest) = tr.model()
    assert (round(executed, 3), round(slowest, 3)) == (0.685, 0.738)
    assert [round(per[j][1], 2) for j in range(1, 12)] == [0.31, 0.35, 0.50, 0.47, 0.67, 0.78, 0.61, 0.85, 0.78, 0.86, 0.88]
    _, (executed_id, slowest_id) = TileRows(hb, place=range(8)).model()
    assert executed_id == executed and round(slowest_id, 3) == 0.847
    assert TileRows.wave_blocks(255) == [9, 9, 9, 9] and TileRows.wave_blocks(0) == [0, 0, 0, 0]


@pytest.mark.parametrize("name", list(OLDER_TABLES))
def test_older_tables_are_unchanged_by_the_tile_rows(name):
    hb, rg, pc = _tables(name)
    pc_before = (pc.has.copy(), pc.perm.copy(), pc.first_chunk.copy(), pc.mask.copy())
    assert hb.tile_rows() is not None
    assert _digest(hb, rg) == OLDER_TABLES[name]
    assert all(np.array_equal(a, b) for a, b in zip(pc_before, (pc.has, pc.perm, pc.first_chunk, pc.mask)))
    # the layout struct has the new fields behind the row groups' rg_zf, the schedule its switch behind regroup_rows: what was last
    # in both stays last; the plan field is appended
    from theseus_amd import _lib
    names = [f for f, _ in _lib.HBlockLayout._fields_]
    k = names.index("tr_tile_host")
    assert names[k - 1:k + 8] == ["rg_zf", "tr_tile_host", "tr_perm16", "tr_mask16", "th_tile_host", "th_perm32", "th_mask32", "th_k0h",
                                  "rg0_rows"] and names[-1] == "row_first"
    sched = [f for f, _ in _lib.CholSchedule._fields_]
    assert sched[-4:] == ["regroup_rows", "sort_tile_rows", "skip_zero_solves", "sort_pair_columns"]
    assert [f for f, _ in _lib.CholPlanInfo._fields_][-2:] == ["sort_pair_columns", "sort_tile_rows"]


def test_plan_reports_sorted_rows_and_their_switches():
    from theseus_amd import _lib
    from theseus_amd.kernels import chol_plan
    import torch
    hb, tr = _tr("headline")
    layout = hb.on("cpu").c      # (the plan reads which tables are set, never their contents)

    def plan(B=4096, dtype=torch.float32, layout=layout, **kw):
        s = _lib.CholSchedule(*([-1] * len(_lib.CholSchedule._fields_)))
        for k, v in kw.items():
            setattr(s, k, v)
        return chol_plan(6 * hb.nvars, hb.ntiles * TILE, B, dtype, layout=layout, schedule=s)
    assert plan()["sort_tile_rows"] == 1 and plan()["split_diag"] == 1 and plan()["sort_pair_columns"] == 1
    assert plan(sort_tile_rows=0)["sort_tile_rows"] == 0 and plan(sort_tile_rows=0)["sort_pair_columns"] == 1
    assert plan(sort_pair_columns=0)["sort_tile_rows"] == 1
    assert plan(regroup_rows=0)["sort_tile_rows"] == 0
    assert plan(skip_zero_blocks=0)["sort_tile_rows"] == 0
    assert plan(B=1016)["sort_tile_rows"] == 1 and plan(B=1016)["split_diag"] == 0          # the fused diagonal kernel: head tiles alone
    assert plan(dtype=torch.float64)["sort_tile_rows"] == 0
    assert plan(B=8)["sort_tile_rows"] == 0                      # (right-looking)

    def without(*fields):
        bare = _lib.HBlockLayout()
        for f, _ in _lib.HBlockLayout._fields_:
            setattr(bare, f, getattr(layout, f))
        for f in fields:
            setattr(bare, f, None)
        return bare
    assert plan(layout=without("tr_mask16"))["sort_tile_rows"] == 1                          # the head tiles' tables are still there
    assert plan(layout=without("th_k0h"))["sort_tile_rows"] == 1 and plan(B=1016, layout=without("th_k0h"))["sort_tile_rows"] == 0
    assert plan(layout=without("tr_mask16", "th_mask32"))["sort_tile_rows"] == 0
