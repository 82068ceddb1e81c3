"""CPU-side (-m "not gpu") checks of thx_chol_solve_multi_sparse: every bad argument is refused on the host before any launch, by its
message; a HipSparseCholeskySolver on a kernel set without the kernel keeps refusing blocks of right-hand sides."""
import ctypes

import pytest
import torch

from tests.test_cabi_and_host import lib_path  # noqa: F401  (the session fixture that builds)

ARGS = ("L", "ld", "n", "B", "Winv", "rhs", "x", "nrhs", "ldv", "bstride", "which", "pattern", "tile_row0", "dtype", "stream")


def test_bad_arguments_are_refused_before_any_launch(lib_path):  # noqa: F811
    from theseus_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    pat = _lib.TilePattern()
    pat.ntiles, pat.nslots, pat.row_ptr, pat.row_tile, pat.row_slot = 1, 1, 4096, 4096, 4096
    ok = dict(L=p, ld=32, n=20, B=2, Winv=p, rhs=p, x=p, nrhs=5, ldv=20, bstride=100, which=0, pattern=ctypes.byref(pat),
              tile_row0=None, dtype=0, stream=None)

    def refused(text, **kw):
        a = dict(ok, **kw)
        return lib.thx_chol_solve_multi_sparse(*[a[k] for k in ARGS]) == -1 and \
            lib.thx_last_error().startswith(b"thx_chol_solve_multi_sparse") and text in lib.thx_last_error()
    for name in ("L", "Winv", "rhs", "x", "pattern"):
        assert refused(b"null pointer", **{name: None}), name
    assert refused(b"n>0", n=0) and refused(b"B>0", B=0)
    for ld in (33, 16, -32):                       # not a frame the factorisation accepts
        assert refused(b"ld", ld=ld), ld
    assert refused(b"tile_row0", tile_row0=p)      # padded tiles on a dense frame
    assert refused(b"nrhs < 1", nrhs=0) and refused(b"nrhs < 1", nrhs=-4)
    assert refused(b"ldv < n", ldv=19)
    assert refused(b"bstride < nrhs * ldv", bstride=99)
    assert refused(b"bstride < nrhs * ldv", ldv=2 ** 62, bstride=2 ** 63 - 1)
    assert refused(b"which", which=-1) and refused(b"which", which=3)
    assert refused(b"dtype", dtype=7)
    assert refused(b"aligned", L=ctypes.c_void_p(4100)) and refused(b"aligned", Winv=ctypes.c_void_p(4104))
    assert refused(b"grid limit", B=64, nrhs=2 ** 31 - 1, bstride=2 ** 63 - 1)
    assert refused(b"not this matrix's", n=200, ld=224)   # one tile cannot hold 200 rows, with or without a table
    assert refused(b"not this matrix's", n=200, ld=0, tile_row0=p)
    pat.nslots = 0
    assert refused(b"nslots", ld=0)                # a tile-packed factor with fewer slots than diagonal tiles
    pat.nslots, pat.row_slot = 1, None
    assert refused(b"incomplete tile pattern", ld=0)


def test_a_kernel_set_without_the_kernel_leaves_the_solver_refusing():
    import theseus_amd as th
    from tests.oracle_kernels import OracleKernels
    from theseus_amd.kernels import HipKernels
    assert hasattr(HipKernels, "chol_solve_multi_sparse") and not hasattr(OracleKernels, "chol_solve_multi_sparse")
    dt = torch.float64
    obj = th.Objective(dtype=dt)
    a, b = (th.SE3(tensor=torch.eye(3, 4, dtype=dt).repeat(2, 1, 1), name=name) for name in "ab")
    w = th.ScaleCostWeight(torch.tensor(1.0, dtype=dt))
    obj.add(th.Between(a, b, th.SE3(tensor=torch.eye(3, 4, dtype=dt).repeat(2, 1, 1), name="m"), w, name="ab"))
    obj.add(th.Difference(a, th.SE3(tensor=torch.eye(3, 4, dtype=dt).repeat(2, 1, 1), name="t"), w, name="prior"))
    solver = th.HipSparseCholeskySolver(obj, linearization_kwargs=dict(kernels=OracleKernels()))
    assert solver._apply_multi is None
    for call in (lambda: solver.sample_deltas(3), lambda: solver.marginal_covariance(["a"]),
                 lambda: solver.solve_multi_with_factor(torch.zeros(2, 1, 12, dtype=dt))):
        with pytest.raises(NotImplementedError, match="HipCholeskySolver"):
            call()
