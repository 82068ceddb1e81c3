"""CPU side of the row-envelope solves (thx_hblock_layout.row_first, thx_chol_solve_env / thx_chol_solve_backward_env): the table
against a dense symbolic factorisation of the same pattern, the table on the layout with and without row groups, the ctypes
binding's null-pointer path and the bytes model of tools/model_solve_bytes.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT


def star_topology(P):
    return [(0, k) for k in range(1, P)]


def path_topology(P):
    return [(k - 1, k) for k in range(1, P)]


def topology(name):
    from theseus_amd.utils.synthetic import pose_graph_topology
    return {"p48": lambda: (pose_graph_topology(48, 96, 0), 48), "p70": lambda: (pose_graph_topology(70, 140, 1), 70),
            "path70": lambda: (path_topology(70), 70), "star48": lambda: (star_topology(48), 48),
            "headline": lambda: (pose_graph_topology(256, 1024, 0), 256)}[name]()


def layout(name):
    from theseus_amd.compiler import PoseGraphStructure
    edges, P = topology(name)
    return PoseGraphStructure.build(P, edges, [0], dof=6).hessian_blocks()


def symbolic_factor(hb):
    """Dense boolean right-looking symbolic Cholesky of the layout's pattern at element granularity: (n, n) lower, True = structural
    non-zero of L."""
    d, n = hb.bd, hb.bd * hb.nvars
    S = np.zeros((n, n), bool)
    for a, b in hb.blocks.tolist():
        S[d * a:d * a + d, d * b:d * b + d] = True
    S = np.tril(S | S.T)
    for k in range(n):
        below = np.flatnonzero(S[k + 1:, k]) + k + 1
        S[np.ix_(below, below)] |= below[:, None] >= below[None, :]
    return S


@pytest.mark.parametrize("name", ["p48", "p70", "path70", "star48", "headline"])
def test_row_first_bounds_every_structural_non_zero_of_the_factor(name):
    hb = layout(name)
    n = hb.bd * hb.nvars
    first = hb.row_first
    assert first.dtype == np.int32 and first.shape == (n,)
    S = symbolic_factor(hb)
    cols = np.arange(n)
    for r in range(n):
        nz = cols[S[r]]
        assert nz.size and nz[0] >= first[r], r        # nothing of L left of first[r]
        assert nz[0] // hb.bd == first[r] // hb.bd, r   # and the envelope is exact at variable granularity
    assert (first % hb.bd == 0).all() and (first <= cols).all()
    if name == "star48":
        assert (first == 0).all()                        # nothing may be skipped
    if name == "path70":
        assert (first == np.maximum(cols // 6 - 1, 0) * 6).all()   # one pose back


def test_row_first_is_on_the_layout_with_and_without_row_groups():
    import torch
    from theseus_amd import _lib
    small, big = layout("star48"), layout("headline")
    assert small.row_groups() is None and big.row_groups() is not None
    for hb in (small, big):
        dev = hb.on("cpu")
        assert dev.t["row_first"].dtype == torch.int32 and dev.c.row_first == dev.t["row_first"].data_ptr()
        assert np.array_equal(dev.t["row_first"].numpy(), hb.row_first)
    rg = big.row_groups()
    assert np.array_equal(rg.first, big.row_first)
    assert _lib.HBlockLayout._fields_[-1][0] == "row_first"


def test_env_exports_take_a_null_table_and_validate_like_the_plain_solves():
    """The two new exports are in the ctypes table with the table pointer in front of dtype; a NULL table is accepted (argument checks
    run first, exactly those of the plain solves, and no device is touched)."""
    from ctypes import c_void_p
    from theseus_amd import _lib
    lib = _lib.load()
    for name in ("thx_chol_solve_env", "thx_chol_solve_backward_env"):
        plain = _lib._SIGNATURES[name.replace("_env", "")]
        assert name in _lib.EXPORTED_SYMBOLS and _lib._SIGNATURES[name] == plain[:8] + [c_void_p] + plain[8:]
        fn, fn0 = getattr(lib, name), getattr(lib, name.replace("_env", ""))
        one = c_void_p(16)   # (never dereferenced: the size checks fail first)
        assert fn(None, 128, 128, 1, None, None, None, 128, None, 0, None) != 0
        assert b"null pointer" in lib.thx_last_error()
        assert fn(one, 128, 128, 0, one, one, one, 128, None, 0, None) != 0          # B = 0, NULL table
        msg = lib.thx_last_error()
        assert fn0(one, 128, 128, 0, one, one, one, 128, 0, None) != 0 and lib.thx_last_error() == msg
        assert fn(one, 64, 128, 1, one, one, one, 128, one, 0, None) != 0 and b"bad sizes" in lib.thx_last_error()   # ld < n


def test_python_wrappers_keep_their_names_and_default_to_no_table():
    import inspect
    from theseus_amd.kernels import HipKernels
    for name in ("chol_solve", "chol_solve_backward"):
        p = inspect.signature(getattr(HipKernels, name)).parameters
        assert list(p)[-1] == "row_first" and p["row_first"].default is None


def test_bytes_model_reproduces_the_headline_ratio():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from model_solve_bytes import solve_bytes
    finally:
        sys.path.pop(0)
    first = layout("headline").row_first.astype(np.int64)
    before, after = solve_bytes(first, 4, 64)
    assert before == 66 * 128 * 128 * 4 + 12 * 128 * 128 * 4 == 5111808
    assert after == 3608448 and round(after / before, 3) == 0.706
    b64, a64 = solve_bytes(first, 8, 64)
    assert b64 == 2 * before and round(a64 / b64, 3) == 0.702
    assert solve_bytes(layout("star48").row_first.astype(np.int64), 4, 16) == (
        (128 * 128 + 32 * 256) * 4 + 3 * 65536, (128 * 128 + 32 * 256) * 4 + 3 * 40960)   # rows 128 .. 255 and 256 .. 287, in full
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "model_solve_bytes.py")], check=True, capture_output=True, text=True).stdout
    assert "fp32   64-byte units:    5111808 ->    3608448 bytes per problem, ratio 0.706" in out
