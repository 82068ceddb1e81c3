"""CPU-side (-m "not gpu"): thx_chol_plan, the host-only query of the schedule a dense-frame factorisation takes.  It runs the
decision function factor_impl itself runs, so these are the paths the GPU schedule tests (tests/test_gpu_chol_schedules.py,
tests/test_gpu_kernels.py, tests/test_gpu_block_hessian.py) rely on reaching -- and the defaults the product runs with."""
import ctypes

import pytest
import torch

F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def plan():
    from theseus_amd import build
    build.build(verbose=False)  # hipcc cross-compiles gfx950 without a GPU; no-op when up to date
    from theseus_amd import _lib
    from theseus_amd.kernels import chol_plan

    def go(n, ld, B, dtype, layout=None, damping=True, rhs=True, ldv=None, **fields):
        s = _lib.CholSchedule(*([-1] * len(_lib.CholSchedule._fields_)))
        for k, v in fields.items():
            setattr(s, k, v)
        return chol_plan(n, ld, B, dtype, damping=damping, rhs=rhs, ldv=ldv, layout=layout, schedule=s)
    return go


def layout(n, max_tile_pieces=10, bd=6, diag_blk=True):
    from theseus_amd import _lib
    c = _lib.HBlockLayout()
    c.bd, c.nvars, c.ntiles, c.max_tile_pieces = bd, n // bd, (n + 127) // 128, max_tile_pieces
    c.diag_blk = 16 if diag_blk else None          # (only its presence is read: the plan touches no device memory)
    return c


def test_defaults_by_dtype_and_batch(plan):
    # right-looking up to 64 (fp32) / 40 (fp64) problems at 12 block columns, mode 1 resp. 2
    for B in (1, 8, 64):
        p = plan(1536, 1536, B, F32)
        assert p["right_looking"] == 1 and p["right_looking_mode"] == 1 and p["column_pairs"] == 0, (B, p)
    for B in (1, 8, 40):
        p = plan(1536, 1536, B, F64)
        assert p["right_looking"] == 1 and p["right_looking_mode"] == 2 and p["f64_half_cols"] == 0 and p["f64_wide_cols"] == 0
    assert plan(1536, 1536, 65, F32)["right_looking"] == 0 and plan(1536, 1536, 41, F64)["right_looking"] == 0
    assert plan(3072, 3072, 32, F64)["right_looking"] == 1 and plan(3072, 3072, 33, F64)["right_looking"] == 0
    # the column-pair floor: 128 problems
    assert plan(1536, 1536, 127, F32)["column_pairs"] == 0 and plan(1536, 1536, 128, F32)["column_pairs"] == 1
    assert plan(1536, 1536, 128, F64)["column_pairs"] == 0
    # fp64, column by column: half tiles for the first 8 block columns, eight waves for the other 3 with off-diagonal tiles
    p = plan(1536, 1536, 128, F64)
    assert (p["f64_half_cols"], p["f64_wide_cols"]) == (8, 3)
    # the split diagonal phase from 2048 problems, two streams from 1024
    assert plan(260, 288, 1024, F32)["nparts"] == 2 and plan(260, 288, 1023, F32)["nparts"] == 1
    assert plan(260, 288, 2048, F64)["split_diag"] == 1 and plan(260, 288, 2047, F64)["split_diag"] == 0


def test_right_looking_needs_whole_tiles_in_the_frame(plan):
    # the product's frames are ld = round_up(n, 32): n = 366 / 1530 are whole tiles, n = 600 / 1290 are not
    assert plan(366, 384, 8, F32)["right_looking"] == 1 and plan(1530, 1536, 8, F64)["right_looking"] == 1
    assert plan(600, 608, 8, F32)["right_looking"] == 0 and plan(1290, 1312, 8, F64)["right_looking"] == 0
    assert plan(1290, 1408, 8, F32)["right_looking"] == 1 and plan(384, 416, 8, F64)["right_looking"] == 1
    assert plan(258, 288, 8, F32)["right_looking"] == 0                       # (fewer than three block columns)
    assert plan(384, 384, 8, F32, split_diag_min_batch=0)["right_looking"] == 0   # (the split diagonal phase is left-looking)


def test_schedule_fields_reach_the_plan(plan):
    for m in (0, 1, 2):
        for dt in (F32, F64):
            p = plan(1536, 1536, 40, dt, right_looking_mode=m, right_looking_max_batch=64)
            assert p["right_looking"] == 1 and p["right_looking_mode"] == m
    assert plan(384, 384, 3, F32, right_looking_mode=7)["right_looking_mode"] == 1   # (> 2: mode 1, as THX_CHOL_RL_LOOKAHEAD)
    assert plan(1536, 1536, 8, F32, right_looking_max_batch=0)["right_looking"] == 0
    assert plan(1536, 1536, 130, F32, right_looking_max_batch=130)["right_looking"] == 1
    # the pair kernel below 128 problems: needs the right-looking schedule off (it comes first)
    p = plan(700, 704, 9, F32, column_pairs_min_batch=0)
    assert p["column_pairs"] == 1 and p["right_looking"] == 0                 # (700: the frame is not whole tiles)
    p = plan(1536, 1536, 8, F32, column_pairs_min_batch=0)
    assert p["column_pairs"] == 0 and p["right_looking"] == 1
    p = plan(1536, 1536, 8, F32, column_pairs_min_batch=0, right_looking_max_batch=0)
    assert p["column_pairs"] == 1 and p["right_looking"] == 0
    assert plan(1536, 1536, 8, F32, column_pairs_min_batch=0, right_looking_max_batch=0, column_pairs=0)["column_pairs"] == 0
    assert plan(1536, 1536, 130, F32, column_pairs_min_batch=131)["column_pairs"] == 0
    # the fp64 off-diagonal kernels per setting (the bit-identity test's settings, 12 block columns)
    for wide, half, exp in ((0, 0, (0, 0)), (1, 0, (0, 1)), (3, 0, (0, 3)), (12, 0, (0, 11)), (0, 1, (1, 0)), (0, 5, (5, 0)),
                            (0, 12, (11, 0)), (12, 4, (4, 7)), (-1, -1, (8, 3))):
        p = plan(1536, 1536, 2, F64, f64_wide_max_ktiles=wide, f64_half_max_ktiles=half, right_looking_max_batch=0)
        assert (p["f64_half_cols"], p["f64_wide_cols"]) == exp, (wide, half, p)


def test_forward_substitution_and_block_layouts(plan):
    # the right-looking schedule fuses the forward substitution only for 16-byte vector rows
    assert plan(384, 384, 8, F32, ldv=384)["forward_fused"] == 1
    assert plan(366, 384, 8, F32)["forward_fused"] == 0 and plan(366, 384, 8, F32, ldv=368)["forward_fused"] == 1
    assert plan(366, 384, 8, F32, rhs=False)["forward_fused"] == 0
    assert plan(600, 608, 8, F32)["forward_fused"] == 1                          # (left-looking: always in chol_diag)
    # block-compact H: the matrix-core scatter (few pieces per tile) keeps the fp64 half / eight-wave kernels, the LDS gather does not
    n = 1536
    p = plan(n, n, 128, F64, layout=layout(n))
    assert (p["f64_half_cols"], p["f64_wide_cols"]) == (8, 3)
    p = plan(n, n, 128, F64, layout=layout(n), hb_scatter_max_pieces=0)
    assert (p["f64_half_cols"], p["f64_wide_cols"]) == (0, 0)
    assert plan(n, n, 128, F64, layout=layout(n, max_tile_pieces=80))["f64_half_cols"] == 0
    # right-looking with damping needs the layout's diagonal block table
    assert plan(n, n, 8, F32, layout=layout(n))["right_looking"] == 1
    assert plan(n, n, 8, F32, layout=layout(n, diag_blk=False))["right_looking"] == 0
    assert plan(n, n, 8, F32, layout=layout(n, diag_blk=False), damping=False)["right_looking"] == 1
    assert plan(n, n, 128, F32, layout=layout(n), column_pairs_min_batch=-1)["column_pairs"] == 1


def test_plan_rejects_bad_arguments(plan):
    from theseus_amd import _lib
    lib = _lib.load()
    out = _lib.CholPlanInfo()
    assert lib.thx_chol_plan(100, 96, 1, 0, 0, 0, 100, None, None, ctypes.byref(out)) != 0 and b"ld" in lib.thx_last_error()
    assert lib.thx_chol_plan(100, 128, 1, 5, 0, 0, 100, None, None, ctypes.byref(out)) != 0 and b"dtype" in lib.thx_last_error()
    assert lib.thx_chol_plan(100, 128, 1, 0, 0, 1, 99, None, None, ctypes.byref(out)) != 0
    assert lib.thx_chol_plan(100, 128, 1, 0, 0, 0, 100, None, None, None) != 0
    assert lib.thx_chol_plan(100, 128, 1, 0, 0, 0, 100, ctypes.byref(layout(1536)), None, ctypes.byref(out)) != 0
    assert lib.thx_chol_plan(100, 128, 1, 0, 0, 0, 100, None, None, ctypes.byref(out)) == 0 and out.right_looking == 0
