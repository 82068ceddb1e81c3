"""Host tables of the zero solves of the fp32 column pairs (thx_hblock_layout.rg_zf / rg0_*, thx_chol_schedule.skip_zero_solves;
theseus_amd/compiler.py:RowGroups): a first non-zero chunk per 32-slot strip (= wave) of every row group, and pair 0's rows in
groups of their own.  No GPU: numpy only, plus the host-only plan query."""
import numpy as np
import pytest

from tests.test_row_groups_host import _case

TILE = 128
CASES = ["headline", "p125", "chain250", "hub125", "p64"]
_CACHE = {}


def _tables(name):
    if name not in _CACHE:
        from theseus_amd.compiler import PoseGraphStructure
        from theseus_amd.utils.synthetic import pose_graph_topology
        edges, P = (pose_graph_topology(64, 128, 0), 64) if name == "p64" else _case(name)
        hb = PoseGraphStructure.build(P, edges, [0], dof=6).hessian_blocks()
        _CACHE[name] = (hb, hb.row_groups(), 6 * P)
    return _CACHE[name]


def _first_of_L(hb):
    """First non-zero column of every row of L, from a numpy symbolic factorisation at variable granularity (column k's structure
    below its first sub-diagonal non-zero p is added to column p) -- as tests/test_row_groups_host.py."""
    P = hb.nvars
    S = np.zeros((P, P), bool)
    for a, b in hb.blocks.tolist():
        S[a, b] = True
    for k in range(P):
        below = np.nonzero(S[k + 1:, k])[0] + k + 1
        if below.size > 1:
            S[below[1:], below[0]] = True
    return np.repeat(6 * np.argmax(S, axis=1), 6)


@pytest.mark.parametrize("name", CASES)
def test_pair_zero_groups_list_every_row_below_the_pair_once(name):
    hb, rg, n = _tables(name)
    assert rg is not None and rg.ngroups0 > 0 and rg.group_ptr[1] == 0     # (the shared tables keep pair 0 empty)
    below = np.arange(2 * TILE, n)
    assert rg.ngroups0 == (below.size + TILE - 1) // TILE and rg.rows0.shape == (rg.ngroups0, TILE) and rg.zf0.shape == (rg.ngroups0, 4)
    slots = rg.rows0.reshape(-1)
    assert np.array_equal(np.sort(slots[:below.size]), below) and (slots[below.size:] == -1).all()
    assert rg.zf.shape == (rg.ngroups, 4)
    if name == "p64":
        assert rg.ngroups == 0 and rg.ngroups0 == 1


@pytest.mark.parametrize("name", CASES)
def test_no_structural_nonzero_left_of_a_strips_first_chunk(name):
    hb, rg, n = _tables(name)
    firstL = _first_of_L(hb)
    assert np.array_equal(firstL, rg.first)
    sets = [(0, rg.rows0, rg.zf0, np.zeros(rg.ngroups0, np.int32))]
    for jp in range(rg.npairs):
        g0, g1 = int(rg.group_ptr[jp]), int(rg.group_ptr[jp + 1])
        sets.append((2 * jp, rg.rows[g0:g1], rg.zf[g0:g1], rg.k0[g0:g1]))
    strips = late = 0
    for j, rows, zf, k0 in sets:
        for g in range(rows.shape[0]):
            for w in range(4):
                r = rows[g, 32 * w:32 * w + 32]
                r = r[r >= 0]
                if r.size == 0:
                    assert zf[g, w] >= 4 * j + 8
                    continue
                assert (firstL[r] >= 32 * zf[g, w]).all() and zf[g, w] == firstL[r].min() // 32, (j, g, w)
                assert zf[g, w] >= k0[g]
                strips += 1
                late += int(zf[g, w] > k0[g])
            assert k0[g] == min(int(zf[g].min()), 4 * j)      # (what the kernel derives when it has the strips' table)
    assert strips > 0 and late > 0


@pytest.mark.parametrize("name", CASES)
def test_pair_zero_piece_tables_reproduce_the_dense_rows(name):
    hb, rg, n = _tables(name)
    ld = hb.ntiles * TILE
    rng = np.random.default_rng(5)
    H = np.zeros((2, n, n))
    for a, b in hb.blocks.tolist():
        H[:, 6 * a:6 * a + 6, 6 * b:6 * b + 6] = rng.standard_normal((2, 6, 6))
    H = np.tril(H)
    want = np.zeros_like(H)
    want[:, 2 * TILE:, :2 * TILE] = H[:, 2 * TILE:, :2 * TILE]
    assert want.any()
    got = rg.expand0(hb.pack_dense(H), ld)
    assert np.array_equal(got[:, :n, :n], want) and not got[:, n:].any() and not got[:, :, n:].any()
    per = np.diff(rg.tile_ptr0)
    assert per.size == 2 * rg.ngroups0 and per.max() == rg.max_tile_pieces0 and rg.tile_ptr0[-1] == rg.piece_blk0.size == rg.piece_rc0.size


def test_headline_model_gives_the_left_out_shares():
    """The model behind the change, from the real tables (tools/model_row_groups.py prints it): 30.7 % of the substitution and
    coupling products and 7.9 % of today's K-loop products are left out, within 2 points (the straddling rule moves a few rows)."""
    hb, rg, _ = _tables("headline")
    model = rg.zero_solve_model(hb.l_mask())
    tot = np.sum([list(r["solve"] + r["kloop"]) for r in model.values()], axis=0)
    print("per pair", model, "totals (solve today, proposed, K-loop today, proposed)", tot.tolist())
    assert tot[0] == 4320 and model[0]["solve"][0] == 1440 and model[0]["kloop"] == (0, 0)
    assert abs(100 * (1 - tot[1] / tot[0]) - 30.7) <= 2.0
    assert abs(100 * (1 - tot[3] / tot[2]) - 7.9) <= 2.0
    assert model[6]["solve"] == (576, 576) and model[8]["solve"] == (288, 288)


def test_small_graph_has_four_different_wave_states_in_one_group():
    """64 poses / 128 edges (n = 384: three block columns, pair 0 only, one group): no skip, a partial X0, X0 = 0, and X0 = 0 with a
    partial X1 -- all four in one workgroup."""
    hb, rg, n = _tables("p64")
    assert n == 384 and hb.ntiles == 3 and rg.ngroups0 == 1
    z = np.clip(rg.zf0[0], 0, 8).tolist()
    print("leading zero sub-blocks per wave", z)
    assert z == [0, 2, 4, 7]


def test_plan_reports_the_switch():
    from theseus_amd import _lib
    from theseus_amd.kernels import chol_plan
    import torch
    hb, rg, n = _tables("headline")
    layout = hb.on("cpu").c      # (the plan reads which tables are set, never their contents)

    def plan(B=4096, dtype=torch.float32, layout=layout, n=n, nt=hb.ntiles, **kw):
        s = _lib.CholSchedule(*([-1] * len(_lib.CholSchedule._fields_)))
        for k, v in kw.items():
            setattr(s, k, v)
        return chol_plan(n, nt * TILE, B, dtype, layout=layout, schedule=s)
    assert plan()["skip_zero_solves"] == 1 and plan()["regroup_rows"] == 1
    assert plan(skip_zero_solves=0)["skip_zero_solves"] == 0 and plan(skip_zero_solves=0)["regroup_rows"] == 1
    assert plan(regroup_rows=0)["skip_zero_solves"] == 0
    assert plan(skip_zero_blocks=0)["skip_zero_solves"] == 0
    assert plan(column_pairs=0)["skip_zero_solves"] == 0
    assert plan(dtype=torch.float64)["skip_zero_solves"] == 0
    assert plan(B=8)["skip_zero_solves"] == 0                      # (right-looking)
    assert plan(hb_scatter_max_pieces=0)["skip_zero_solves"] == 1  # (the LDS gather has no piece limit)
    # a layout without the new tables
    bare = _lib.HBlockLayout()
    for f, _ in _lib.HBlockLayout._fields_:
        setattr(bare, f, getattr(layout, f))
    bare.rg_zf = None
    bare.rg0_rows = None
    assert plan(layout=bare)["skip_zero_solves"] == 0 and plan(layout=bare)["regroup_rows"] == 1
    # pair 0's groups alone switch it on (three block columns: no group with a K-loop), the strips' table alone as well
    hb3, rg3, n3 = _tables("p64")
    assert plan(B=128, layout=hb3.on("cpu").c, n=n3, nt=3)["skip_zero_solves"] == 1
    assert plan(B=128, layout=hb3.on("cpu").c, n=n3, nt=3)["regroup_rows"] == 0
    only_zf = _lib.HBlockLayout()
    for f, _ in _lib.HBlockLayout._fields_:
        setattr(only_zf, f, getattr(layout, f))
    only_zf.rg0_ngroups = 0
    assert plan(layout=only_zf)["skip_zero_solves"] == 1
