"""Host tables of the regrouped fp32 column pairs (thx_hblock_layout.rg_*, theseus_amd/compiler.py:RowGroups): the rows below
every column pair sorted by their first non-zero column and cut into groups of 128, a first K-loop chunk per group, and the
group's pieces of H.  No GPU: numpy only, plus the host-only plan query."""
import numpy as np
import pytest

TILE = 128


def _hub_topology():
    """125 poses: the odometry chain, every pose >= 86 tied to three poses in 43..84, a few of them also to poses < 20."""
    edges = [(k - 1, k) for k in range(1, 125)]
    for p in range(86, 125):
        edges += [(43 + (7 * p + 13 * t) % 42, p) for t in range(3)]
    edges += [(p % 20, p) for p in (90, 97, 104, 111, 118)]
    return sorted(set(edges))


def _case(name):
    from theseus_amd.utils.synthetic import pose_graph_topology
    if name == "headline":
        return pose_graph_topology(256, 1024, 0), 256
    if name == "p125":
        return pose_graph_topology(125, 500, 0), 125
    if name == "chain250":   # n = 1500: the last tile is partial
        return [(k - 1, k) for k in range(1, 250)], 250
    if name == "hub125":
        return _hub_topology(), 125
    raise KeyError(name)


_CACHE = {}


def _tables(name):
    if name not in _CACHE:
        from theseus_amd.compiler import PoseGraphStructure
        edges, P = _case(name)
        hb = PoseGraphStructure.build(P, edges, [0], dof=6).hessian_blocks()
        _CACHE[name] = (hb, hb.row_groups(), 6 * P)
    return _CACHE[name]


CASES = ["headline", "p125", "chain250", "hub125"]


@pytest.mark.parametrize("name", CASES)
def test_every_pair_lists_the_rows_below_it_once(name):
    hb, rg, n = _tables(name)
    assert rg is not None and rg.npairs == (hb.ntiles - 1) // 2 and rg.group_ptr[0] == 0
    assert rg.group_ptr[1] == 0                                  # pair j = 0 has no K-loop: natural tiles
    some = False
    for jp in range(rg.npairs):
        g0, g1 = int(rg.group_ptr[jp]), int(rg.group_ptr[jp + 1])
        if g1 == g0:
            continue
        j = 2 * jp
        below = np.arange((j + 2) * TILE, n)
        assert g1 - g0 == (below.size + TILE - 1) // TILE
        slots = rg.rows[g0:g1].reshape(-1)
        assert np.array_equal(np.sort(slots[:below.size]), below) and (slots[below.size:] == -1).all()
        k0 = rg.k0[g0:g1]
        assert k0.max() > 0 and (k0 >= 0).all() and (k0 <= 4 * j).all()
        # groups in ascending order of their first non-zero column: the longest K-loops are dispatched first
        assert (np.diff(k0) >= 0).all()
        some = True
    assert some


@pytest.mark.parametrize("name", CASES)
def test_no_structural_nonzero_left_of_a_groups_first_chunk(name):
    """Against a numpy symbolic factorisation at variable granularity (column k's structure below its first sub-diagonal
    non-zero p is added to column p): no row of a group has a non-zero of L in a chunk in front of the group's k0."""
    hb, rg, n = _tables(name)
    P = hb.nvars
    S = np.zeros((P, P), bool)
    for a, b in hb.blocks.tolist():
        S[a, b] = True
    for k in range(P):
        below = np.nonzero(S[k + 1:, k])[0] + k + 1
        if below.size > 1:
            S[below[1:], below[0]] = True
    firstL = np.repeat(6 * np.argmax(S, axis=1), 6)      # first non-zero column of every row of L
    assert np.array_equal(firstL, rg.first)              # (the envelope: L's rows begin where H's do)
    for g in range(rg.ngroups):
        rows = rg.rows[g][rg.rows[g] >= 0]
        assert (firstL[rows] >= 32 * rg.k0[g]).all(), g


@pytest.mark.parametrize("name", CASES)
def test_group_piece_tables_reproduce_the_dense_rows(name):
    hb, rg, n = _tables(name)
    ld = hb.ntiles * TILE
    rng = np.random.default_rng(5)
    H = np.zeros((2, n, n))
    for a, b in hb.blocks.tolist():
        H[:, 6 * a:6 * a + 6, 6 * b:6 * b + 6] = rng.standard_normal((2, 6, 6))
    H = np.tril(H)
    want = np.zeros_like(H)
    for jp in range(rg.npairs):
        if rg.group_ptr[jp + 1] > rg.group_ptr[jp]:
            r0, c0 = (2 * jp + 2) * TILE, 2 * jp * TILE
            want[:, r0:, c0:c0 + 2 * TILE] = H[:, r0:, c0:c0 + 2 * TILE]
    assert want.any()
    got = rg.expand(hb.pack_dense(H), ld)
    assert np.array_equal(got[:, :n, :n], want) and not got[:, n:].any() and not got[:, :, n:].any()
    # the tables' own bounds: two runs per group, the maximum the plan compares with the scatter limit
    per = np.diff(rg.tile_ptr)
    assert per.size == 2 * rg.ngroups and per.max() == rg.max_tile_pieces and rg.tile_ptr[-1] == rg.piece_blk.size == rg.piece_rc.size


def test_headline_tables_give_the_models_skipped_fraction():
    hb, rg, _ = _tables("headline")
    per, total = rg.skipped_fraction(hb.l_mask())
    print("skipped fraction per pair", per, "all pairs", total)
    assert abs(total - 0.298) <= 0.005
    assert per[0] == 0.0 and per[2] > per[4] > per[6] > per[8] > 0.0


def test_hub_graph_has_an_empty_k_loop_and_more_pieces_than_the_registers_hold():
    """The GPU test's hub case is what it is meant to be: one group starts at the END of its K-loop (zero iterations) and one
    group's pieces of both column tiles exceed the 42 (2 x 3 x 256 / 36) that chol_offdiag2_f32_kernel holds in registers."""
    hb, rg, _ = _tables("hub125")
    g0, g1 = int(rg.group_ptr[1]), int(rg.group_ptr[2])
    assert g1 - g0 == 2 and rg.k0[g0] == 0 and rg.k0[g1 - 1] == 8
    both = np.diff(rg.tile_ptr)[2 * g0:2 * g1].reshape(-1, 2).sum(1)
    assert both.max() > 42 and rg.max_tile_pieces <= 64


def test_plan_reports_regrouping_and_its_switches():
    from theseus_amd import _lib
    from theseus_amd.kernels import chol_plan
    import torch
    hb, rg, n = _tables("headline")
    layout = hb.on("cpu").c      # (the plan reads which tables are set, never their contents)

    def plan(B=4096, dtype=torch.float32, layout=layout, **kw):
        s = _lib.CholSchedule(*([-1] * len(_lib.CholSchedule._fields_)))
        for k, v in kw.items():
            setattr(s, k, v)
        return chol_plan(n, hb.ntiles * TILE, B, dtype, layout=layout, schedule=s)
    assert plan()["regroup_rows"] == 1 and plan()["column_pairs"] == 1
    assert plan(regroup_rows=0)["regroup_rows"] == 0
    assert plan(skip_zero_blocks=0)["regroup_rows"] == 0
    assert plan(column_pairs=0)["regroup_rows"] == 0
    assert plan(dtype=torch.float64)["regroup_rows"] == 0
    assert plan(B=8)["regroup_rows"] == 0                        # (right-looking)
    assert plan(hb_scatter_max_pieces=0)["regroup_rows"] == 1    # (the LDS gather has no piece limit)
    assert plan(hb_scatter_max_pieces=rg.max_tile_pieces - 1)["regroup_rows"] == int(
        _lib.max_offdiag_tile_pieces(hb.tile_ptr, hb.ntiles) > rg.max_tile_pieces - 1)
    # a layout without the tables: no regrouping
    bare = _lib.HBlockLayout()
    for f, _ in _lib.HBlockLayout._fields_:
        setattr(bare, f, getattr(layout, f))
    bare.rg_rows = None
    assert plan(layout=bare)["regroup_rows"] == 0
